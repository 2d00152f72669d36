// ofdm_capi.cpp — implementation of include/ofdm_mi355x.h (the C-ABI drop-in
// boundary): the entry points. Host side: argument checks and kernel dispatch
// on a context that ofdm_create.cpp built (config parsing, validation and the
// constant tables are there; the stream receiver is ofdm_stream_call.cpp).
// Every compute entry point launches HIP kernels; there is no CPU compute path.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <mutex>
#include <cstring>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ofdm_mi355x.h"

// RCCL's types and enum values for the one collective (ofdm_reduce_counters):
// from its header where the build host has it; the library itself is loaded
// at first use, so the core library neither links RCCL nor needs it to run
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
static constexpr int kRcclInt64 = ncclInt64, kRcclSum = ncclSum;
#else
static constexpr int kRcclInt64 = 4, kRcclSum = 0;  // rccl.h: ncclInt64, ncclSum (header absent at build time)
#endif
#include "ofdm_csi.hpp"
#include "ofdm_ctx.hpp"
#include "ofdm_internal.hpp"
#include "ofdm_mac.hpp"
#include "ofdm_sync.hpp"

namespace {
thread_local std::string g_err;
}

// (declared in ofdm_ctx.hpp: ofdm_stream_call.cpp reports errors the same way)
int ofdm::fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int ofdm::hip_fail(hipError_t e, const char* what)
{
    return fail(OFDM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

using ofdm::aligned16;
using ofdm::capture_refused;
using ofdm::capturing;
using ofdm::cfo_plan;
using ofdm::fail;
using ofdm::grow;
using ofdm::grow_host;
using ofdm::hip_fail;
using ofdm::initial_state;

// ---- the other helpers that ofdm_ctx.hpp declares ----

// True while `st` is being captured into a hipGraph. Asked only on the paths
// that are about to allocate, copy from pageable memory or synchronise (none
// of which a capture allows), so that they can refuse before they break the
// capture; the launches themselves never ask.
bool ofdm::capturing(hipStream_t st)
{
    hipStreamCaptureStatus s = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &s) != hipSuccess) {
        (void)hipGetLastError();  // (the legacy stream beside another stream's capture: not capturing)
        return false;
    }
    return s != hipStreamCaptureStatusNone;
}

int ofdm::capture_refused(const char* what)
{
    return fail(OFDM_ERR_UNSUPPORTED, "%s: not possible on a stream that is being captured (make the same call once "
                                      "before the capture)", what);
}

bool ofdm::aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Device scratch that only grows (contents not preserved).
int ofdm::grow(ofdm_ctx* c, ofdm_ctx::Grow& g, size_t need)
{
    if (need <= g.bytes) return OFDM_OK;
    HIP_TRY(hipSetDevice(c->device));
    g.bytes = 0;
    HIP_TRY(g.p.reset());
    HIP_TRY(hipMalloc(g.p.put(), need));
    g.bytes = need;
    return OFDM_OK;
}

// Pinned host staging that only grows (contents not preserved).
int ofdm::grow_host(ofdm_ctx* c, ofdm_ctx::GrowHost& g, size_t need)
{
    if (need <= g.bytes) return OFDM_OK;
    HIP_TRY(hipSetDevice(c->device));
    g.bytes = 0;
    HIP_TRY(g.p.reset());
    HIP_TRY(hipHostMalloc(g.p.put(), need, hipHostMallocDefault));
    g.bytes = need;
    return OFDM_OK;
}

// rx.cpp's initial walk state (rx.cpp:105-114): pos = 0 of a buffer whose
// first output_size samples are the zero header before the first SDR buffer,
// i.e. stream position -output_size in a ring ending at R; the continuous
// walk starts at the stream's first sample.
ofdm_walk_state ofdm::initial_state(const ofdm_ctx* c)
{
    return c->ring > 0 ? ofdm_walk_state{-c->geo.frame_len, c->ring} : ofdm_walk_state{0, 0};
}

extern "C" {

const char* ofdm_last_error(void) { return g_err.c_str(); }
int ofdm_abi_version(void) { return OFDM_MI355X_ABI_VERSION; }

// The rx frame-queue slot of `st` (nullptr: no slot free, static frame order).
static int* rx_queue(ofdm_ctx* c, hipStream_t st)
{
    int free_slot = -1;
    for (int i = 0; i < c->rxq_used; ++i) {
        if (c->rxq_live[i] && c->rxq_stream[i] == st) return c->d_rxq + 16 * i;
        if (!c->rxq_live[i] && free_slot < 0) free_slot = i;
    }
    if (free_slot < 0) {
        if (c->rxq_used == ofdm_ctx::RX_QUEUE_SLOTS) return nullptr;
        free_slot = c->rxq_used++;
    }
    c->rxq_stream[free_slot] = st;
    c->rxq_live[free_slot] = true;
    return c->d_rxq + 16 * free_slot;
}

// ofdm_stream_destroy: the stream's slot becomes free for a later stream (its
// counters are zero once the stream has drained: the last workgroup of every
// rx launch resets them), so a handle value reused by a new stream starts on
// a clean slot and short-lived streams do not use the slots up.
static void rx_queue_release(ofdm_ctx* c, hipStream_t st)
{
    for (int i = 0; i < c->rxq_used; ++i)
        if (c->rxq_live[i] && c->rxq_stream[i] == st) c->rxq_live[i] = false;
}

// A launch that did not start leaves its slot as it was (zero). One that
// faulted poisons the context anyway (HIP errors are sticky); the slot is
// still zeroed so a recovered context starts clean.
static void rx_queue_reset(ofdm_ctx* c, int* q, hipStream_t st)
{
    if (q) (void)hipMemsetAsync(q, 0, 2 * sizeof(int), st);
}

int ofdm_get_geometry(const ofdm_ctx* c, ofdm_geometry* o)
{
    if (!c || !o) return fail(OFDM_ERR_INVALID, "null argument");
    *o = c->geo;
    return OFDM_OK;
}

int ofdm_rx_emit_fast(const ofdm_ctx* c) { return c ? (c->dec_fast ? 1 : 0) : -1; }

int ofdm_tx_sparse(ofdm_ctx* c, int enable, unsigned* masks_out, int* codes_out)
{
    if (!c) return -1;
    if (enable >= 0) c->tx_sparse = enable != 0;
    if (masks_out) std::copy(c->tx_dead.begin(), c->tx_dead.end(), masks_out);
    if (codes_out) std::copy(c->tx_code.begin(), c->tx_code.end(), codes_out);
    return c->tx_sparse && c->d_tx_dead ? 1 : 0;
}

int ofdm_get_t2_symbol(const ofdm_ctx* c, double* o)
{
    if (!c || !o) return fail(OFDM_ERR_INVALID, "null argument");
    std::memcpy(o, c->t2_symbol.data(), c->t2_symbol.size() * sizeof(cd));
    return OFDM_OK;
}

int ofdm_get_preamble(const ofdm_ctx* c, uint8_t* bytes, double* pre, double* modp, double* templ)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    if (bytes) std::memcpy(bytes, c->preamble_bytes.data(), c->preamble_bytes.size());
    if (pre) std::memcpy(pre, c->ofdm_preamble.data(), c->ofdm_preamble.size() * sizeof(cd));
    if (modp) std::memcpy(modp, c->mod_preamble.data(), c->mod_preamble.size() * sizeof(cd));
    if (templ) std::memcpy(templ, c->templ.data(), c->templ.size() * sizeof(cd));
    return OFDM_OK;
}

// ---- memory helpers
int ofdm_device_alloc(ofdm_ctx* c, size_t bytes, void** d)
{
    if (!c || !d) return fail(OFDM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc(d, std::max<size_t>(bytes, 1)));
    return OFDM_OK;
}
int ofdm_device_free(ofdm_ctx* c, void* d)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    if (d) HIP_TRY(hipFree(d));
    return OFDM_OK;
}
int ofdm_memcpy_h2d(ofdm_ctx* c, void* dst, const void* src, size_t n, void* st)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, (hipStream_t)st));
    return OFDM_OK;
}
int ofdm_memcpy_d2h(ofdm_ctx* c, void* dst, const void* src, size_t n, void* st)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, (hipStream_t)st));
    return OFDM_OK;
}
int ofdm_memset_device(ofdm_ctx* c, void* dst, int v, size_t n, void* st)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    HIP_TRY(hipMemsetAsync(dst, v, n, (hipStream_t)st));
    return OFDM_OK;
}
int ofdm_stream_synchronize(ofdm_ctx* c, void* st)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    HIP_TRY(hipStreamSynchronize((hipStream_t)st));
    return OFDM_OK;
}

int ofdm_host_alloc(ofdm_ctx* c, size_t bytes, void** h)
{
    if (!c || !h) return fail(OFDM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostMalloc(h, std::max<size_t>(bytes, 1), hipHostMallocDefault));
    return OFDM_OK;
}
int ofdm_host_free(ofdm_ctx* c, void* h)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    if (h) HIP_TRY(hipHostFree(h));
    return OFDM_OK;
}
int ofdm_stream_create(ofdm_ctx* c, void** st)
{
    if (!c || !st) return fail(OFDM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *st = s;
    return OFDM_OK;
}
int ofdm_stream_destroy(ofdm_ctx* c, void* st)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    if (st) {
        HIP_TRY(hipStreamSynchronize((hipStream_t)st));
        rx_queue_release(c, (hipStream_t)st);
        if (c->call_valid && c->call_stream == (hipStream_t)st) c->call_valid = false;  // drained above
        HIP_TRY(hipStreamDestroy((hipStream_t)st));
    }
    return OFDM_OK;
}
int ofdm_memcpy_d2d(ofdm_ctx* c, void* dst, const void* src, size_t n, void* st)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    if (n) HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, (hipStream_t)st));
    return OFDM_OK;
}
int ofdm_copy(ofdm_ctx* c, void* dst, const void* src, size_t n, void* st)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    if (n && (!dst || !src)) return fail(OFDM_ERR_INVALID, "null argument");
    hipError_t e = ofdm::launch_copy(dst, src, n, (hipStream_t)st);
    if (e != hipSuccess) return hip_fail(e, "copy launch");
    return OFDM_OK;
}
int ofdm_event_create(ofdm_ctx* c, void** ev)
{
    if (!c || !ev) return fail(OFDM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *ev = e;
    return OFDM_OK;
}
int ofdm_event_record(ofdm_ctx* c, void* ev, void* st)
{
    if (!c || !ev) return fail(OFDM_ERR_INVALID, "null argument");
    HIP_TRY(hipEventRecord((hipEvent_t)ev, (hipStream_t)st));
    return OFDM_OK;
}
int ofdm_event_synchronize(ofdm_ctx* c, void* ev)
{
    if (!c || !ev) return fail(OFDM_ERR_INVALID, "null argument");
    HIP_TRY(hipEventSynchronize((hipEvent_t)ev));
    return OFDM_OK;
}
int ofdm_event_destroy(ofdm_ctx* c, void* ev)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    if (ev) HIP_TRY(hipEventDestroy((hipEvent_t)ev));
    return OFDM_OK;
}

static void fill_tx(const ofdm_ctx* c, ofdm::TxArgs& a, const uint8_t* bytes, size_t nframes, double* iq,
                    size_t stride, int16_t* iq16, const ofdm_channel* ch)
{
    a.tab = c->tables(false);
    a.tx_dead = c->tx_sparse ? c->d_tx_dead : nullptr;
    a.bytes = bytes;
    a.iq = reinterpret_cast<double2*>(iq);
    a.iq16 = iq16;
    a.nframes = (long)nframes;
    a.frame_stride = (long)stride;
    a.S = c->S;
    a.D = c->D;
    a.P = c->P;
    a.cp = c->cp;
    a.k = c->k;
    a.bytes_per_frame = c->geo.bytes_per_frame;
    a.pilot_ampl = (double)c->p.pilot_ampl / 1000;
    a.inv_sqrt_n = 1.0 / std::sqrt((double)c->N);
    a.mult = (double)c->p.mult;
    if (ch && ch->noise_std > 0.0) {
        a.noise_scale = ch->noise_std * M_SQRT1_2;
        a.seed = ch->seed;
        a.sample_offset = ch->sample_offset;
    }
}

int ofdm_tx_modulate(ofdm_ctx* c, const uint8_t* bytes, size_t nframes, double* iq_out, size_t frame_stride,
                     int16_t* iq16_out, const ofdm_channel* ch, void* stream)
{
    if (!c || !bytes || !iq_out) return fail(OFDM_ERR_INVALID, "null argument");
    if (frame_stride < (size_t)c->geo.message_len) return fail(OFDM_ERR_INVALID, "frame_stride < message_len");
    if (!aligned16(iq_out)) return fail(OFDM_ERR_INVALID, "iq_out must be 16-byte aligned");
    if (nframes == 0) return OFDM_OK;
    if (nframes * (size_t)c->S > 0x7fffffffu) return fail(OFDM_ERR_INVALID, "too many symbols in one call");
    ofdm::TxArgs a{};
    fill_tx(c, a, bytes, nframes, iq_out, frame_stride, iq16_out, ch);
    hipError_t e = ofdm::launch_tx(c->logn, a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "tx_kernel launch");
    return OFDM_OK;
}

int ofdm_tx_frames(ofdm_ctx* c, const uint8_t* bytes, size_t nframes, double* frames_out, int16_t* frames16_out,
                   void* stream)
{
    if (!c || !bytes || !frames_out) return fail(OFDM_ERR_INVALID, "null argument");
    if (!aligned16(frames_out)) return fail(OFDM_ERR_INVALID, "frames_out must be 16-byte aligned");
    if (nframes == 0) return OFDM_OK;
    ofdm::TxArgs a{};
    fill_tx(c, a, bytes, nframes, frames_out, (size_t)c->geo.frame_len, frames16_out, nullptr);
    a.header = c->d_header;
    a.header_len = (int)(c->t2 + c->geo.preamble_len);
    a.msg_offset = a.header_len;
    hipError_t e = ofdm::launch_tx(c->logn, a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "tx_kernel launch");
    return OFDM_OK;
}

}  // extern "C"

// ofdm_rx_demod / ofdm_rx_demod_i16: exactly one of iq, iq16 is set.
static int rx_demod_impl(ofdm_ctx* c, const double* iq, const int16_t* iq16, size_t nframes, size_t frame_stride,
                         const double* chan, size_t chan_stride, double* constell_out, uint8_t* bytes_out,
                         const uint8_t* ref_bytes, unsigned long long* bit_errors, void* stream,
                         double* read_out = nullptr, const ofdm::SoftArgs* soft = nullptr)
{
    if (!c || (!iq && !iq16)) return fail(OFDM_ERR_INVALID, "null argument");
    if (iq16 && ((uintptr_t)iq16 & 3)) return fail(OFDM_ERR_INVALID, "iq16 must be 4-byte aligned");
    if (frame_stride < (size_t)c->geo.message_len) return fail(OFDM_ERR_INVALID, "frame_stride < message_len");
    if ((iq && !aligned16(iq)) || (chan && !aligned16(chan)) || (constell_out && !aligned16(constell_out)))
        return fail(OFDM_ERR_INVALID, "complex buffers must be 16-byte aligned");
    if ((ref_bytes == nullptr) != (bit_errors == nullptr))
        return fail(OFDM_ERR_INVALID, "ref_bytes and bit_errors go together");
    if (nframes == 0) return OFDM_OK;
    if (nframes > 0x7fffffffu) return fail(OFDM_ERR_INVALID, "too many frames in one call");
    ofdm::RxArgs a{};
    a.tab = c->tables(false);
    a.iq = iq16 ? nullptr : reinterpret_cast<const double2*>(iq);
    a.iq16 = reinterpret_cast<const short2*>(iq16);
    a.nframes = (long)nframes;
    a.frame_stride = (long)frame_stride;
    a.chan = reinterpret_cast<const double2*>(chan);
    a.chan_stride = (long)chan_stride;
    a.constell = reinterpret_cast<double2*>(constell_out);
    a.read_out = reinterpret_cast<double2*>(read_out);
    a.bytes = bytes_out;
    a.ref = ref_bytes;
    a.bit_errors = bit_errors;
    a.S = c->S;
    a.D = c->D;
    a.P = c->P;
    a.seg = c->seg;
    a.cp = c->cp;
    a.k = c->k;
    a.bytes_per_frame = c->geo.bytes_per_frame;
    a.pilot_ampl = (double)c->p.pilot_ampl / 1000;
    a.queue = rx_queue(c, (hipStream_t)stream);
    for (int j = 0; j < 3; ++j) a.dec_tau[j] = c->dec_tau[j];
    a.dec_fast = c->dec_fast;
    const bool fits = c->S <= ofdm::RX_SMAX && c->D <= ofdm::RX_DPT * (c->N / 8);
    if (!fits) {
        if (c->D > ofdm::RX_DPT * (c->N / 8))
            return fail(OFDM_ERR_UNSUPPORTED, "num_data_subc > fft_size/2 is not covered by the rx kernel");
        if (constell_out) {
            a.ystage = a.constell;
        } else {
            const size_t need = nframes * (size_t)c->S * c->D * sizeof(double2);
            if (need > c->d_scratch.bytes && capturing((hipStream_t)stream))
                return capture_refused("growing the staged rx scratch");
            if (int rc = grow(c, c->d_scratch, need)) return rc;
            a.ystage = static_cast<double2*>(c->d_scratch.p.get());
        }
    }
    hipError_t e = soft ? ofdm::launch_rx_soft(c->logn, a, *soft, (hipStream_t)stream)
                        : ofdm::launch_rx(c->logn, a, (hipStream_t)stream, nullptr);
    if (e != hipSuccess) {
        rx_queue_reset(c, a.queue, (hipStream_t)stream);
        return hip_fail(e, "rx_kernel launch");
    }
    return OFDM_OK;
}

// Argument checks shared by the two soft entry points.
static int soft_args_check(const ofdm_ctx* c, double scale, int fmt, const void* llr_out)
{
    if (!c || !llr_out) return fail(OFDM_ERR_INVALID, "null argument");
    if (fmt != OFDM_LLR_F32 && fmt != OFDM_LLR_I8) return fail(OFDM_ERR_INVALID, "fmt is not OFDM_LLR_F32 / OFDM_LLR_I8");
    if (!std::isfinite(scale) || !(scale > 0.0)) return fail(OFDM_ERR_INVALID, "scale must be finite and > 0");
    if (fmt == OFDM_LLR_F32 && ((uintptr_t)llr_out & 3)) return fail(OFDM_ERR_INVALID, "llr_out must be 4-byte aligned");
    if (c->k != 1 && c->k != 2 && c->k != 4 && c->k != 6 && c->k != 8)
        return fail(OFDM_ERR_UNSUPPORTED, "soft demapping covers modType 1, 2, 4, 6, 8 (not %d)", (int)c->k);
    return OFDM_OK;
}

// Channel code: kept bits of the 2*(info_bits + 6) mother bits of one codeword.
static bool fec_rate_ok(int rate) { return rate == OFDM_FEC_R12 || rate == OFDM_FEC_R23 || rate == OFDM_FEC_R34; }

static size_t fec_coded(size_t info_bits, int rate)
{
    const ofdm::FecRate r = ofdm::fec_rate(rate);
    const size_t m = 2 * (info_bits + ofdm::FEC_TAIL);
    return m / r.period * r.kept + (size_t)__builtin_popcount(r.mask & ((1u << (m % r.period)) - 1u));
}

// Interleaver: a block of n positions in c columns with rotation group s.
static bool il_params_ok(size_t n, size_t c, size_t s)
{
    return n >= 8 && n <= (size_t)ofdm::IL_MAX_BLOCK && n % 8 == 0 && c >= 1 && n % c == 0 && s >= 1 &&
           (n / c) % s == 0;
}

// The three interleave entry points: `kind` is ofdm::IL_BITS / IL_I8 / IL_F32.
static int interleave_impl(ofdm_ctx* c, const void* in, int kind, size_t nblocks, size_t n, size_t cols, size_t s,
                           int dir, void* out, void* stream)
{
    if (!c || !in || !out) return fail(OFDM_ERR_INVALID, "null argument");
    if (!il_params_ok(n, cols, s))
        return fail(OFDM_ERR_INVALID, "block_bits=%zu, cols=%zu, s=%zu is no valid interleaver block", n, cols, s);
    if (dir != OFDM_IL_FORWARD && dir != OFDM_IL_INVERSE)
        return fail(OFDM_ERR_INVALID, "dir is not OFDM_IL_FORWARD / OFDM_IL_INVERSE");
    if (kind == ofdm::IL_F32 && (((uintptr_t)in | (uintptr_t)out) & 3))
        return fail(OFDM_ERR_INVALID, "F32 buffers must be 4-byte aligned");
    if (nblocks > (size_t)LONG_MAX / (4 * n)) return fail(OFDM_ERR_INVALID, "nblocks out of range");
    const size_t bytes = kind == ofdm::IL_BITS ? nblocks * n / 8 : kind == ofdm::IL_I8 ? nblocks * n : nblocks * n * 4;
    const uintptr_t a0 = (uintptr_t)in, b0 = (uintptr_t)out;
    if (a0 < b0 + bytes && b0 < a0 + bytes && bytes) return fail(OFDM_ERR_INVALID, "in and out overlap");
    if (nblocks == 0) return OFDM_OK;
    ofdm::IlArgs a{in, out, (long)nblocks, (int)n, (int)cols, (int)s, kind, dir};
    hipError_t e = ofdm::launch_interleave(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "interleave launch");
    return OFDM_OK;
}

extern "C" {

int ofdm_rx_demod(ofdm_ctx* c, const double* iq, size_t nframes, size_t frame_stride, const double* chan,
                  size_t chan_stride, double* constell_out, uint8_t* bytes_out, const uint8_t* ref_bytes,
                  unsigned long long* bit_errors, void* stream)
{
    if (!iq) return fail(OFDM_ERR_INVALID, "null argument");
    return rx_demod_impl(c, iq, nullptr, nframes, frame_stride, chan, chan_stride, constell_out, bytes_out, ref_bytes,
                         bit_errors, stream);
}

int ofdm_rx_demod_i16(ofdm_ctx* c, const int16_t* iq16, size_t nframes, size_t frame_stride, const double* chan,
                      size_t chan_stride, double* constell_out, uint8_t* bytes_out, const uint8_t* ref_bytes,
                      unsigned long long* bit_errors, void* stream)
{
    if (!iq16) return fail(OFDM_ERR_INVALID, "null argument");
    return rx_demod_impl(c, nullptr, iq16, nframes, frame_stride, chan, chan_stride, constell_out, bytes_out,
                         ref_bytes, bit_errors, stream);
}

int ofdm_rx_demod_read(ofdm_ctx* c, const double* iq, size_t nframes, size_t frame_stride, const double* chan,
                       size_t chan_stride, double* read_out, double* constell_out, uint8_t* bytes_out, void* stream)
{
    if (!iq || !chan || !read_out) return fail(OFDM_ERR_INVALID, "null argument");
    if (!aligned16(read_out)) return fail(OFDM_ERR_INVALID, "complex buffers must be 16-byte aligned");
    return rx_demod_impl(c, iq, nullptr, nframes, frame_stride, chan, chan_stride, constell_out, bytes_out, nullptr,
                         nullptr, stream, read_out);
}

int ofdm_demap(ofdm_ctx* c, double* points, size_t n, uint8_t* bytes_out, void* stream)
{
    if (!c || !points || !bytes_out) return fail(OFDM_ERR_INVALID, "null argument");
    hipError_t e = ofdm::launch_demap(reinterpret_cast<double2*>(points), (long)n, c->k, bytes_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "demap launch");
    return OFDM_OK;
}

int ofdm_soft_demap(ofdm_ctx* c, const double* points, size_t n, double scale, int fmt, void* llr_out, void* stream)
{
    if (!c || !points) return fail(OFDM_ERR_INVALID, "null argument");
    if (int rc = soft_args_check(c, scale, fmt, llr_out)) return rc;
    if (!aligned16(points)) return fail(OFDM_ERR_INVALID, "points must be 16-byte aligned");
    hipError_t e = ofdm::launch_soft_demap(reinterpret_cast<const double2*>(points), (long)n, c->k, scale, fmt, llr_out,
                                           (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "soft demap launch");
    return OFDM_OK;
}

int ofdm_soft_demap_csi(ofdm_ctx* c, const double* points, size_t nframes, const double* csi, size_t csi_stride,
                        double scale, const double* frame_scale, int fmt, void* llr_out, void* stream)
{
    if (!c || !points || !csi) return fail(OFDM_ERR_INVALID, "null argument");
    if (int rc = soft_args_check(c, scale, fmt, llr_out)) return rc;
    if (!aligned16(points)) return fail(OFDM_ERR_INVALID, "points must be 16-byte aligned");
    if (((uintptr_t)csi & 7) || ((uintptr_t)frame_scale & 7))
        return fail(OFDM_ERR_INVALID, "csi and frame_scale must be 8-byte aligned");
    if (csi_stride != 0 && csi_stride < (size_t)c->D) return fail(OFDM_ERR_INVALID, "csi_stride < num_data_subc");
    if (nframes > (size_t)LONG_MAX / ((size_t)c->D * c->S * 32)) return fail(OFDM_ERR_INVALID, "nframes out of range");
    if (nframes == 0) return OFDM_OK;
    ofdm::SoftCsiArgs a{};
    a.pts = reinterpret_cast<const double2*>(points);
    a.csi = csi;
    a.frame_scale = frame_scale;
    a.out = llr_out;
    a.nframes = (long)nframes;
    a.csi_stride = (long)csi_stride;
    a.npts = c->D * c->S;
    a.D = c->D;
    a.k = c->k;
    a.fmt = fmt;
    a.scale = scale;
    hipError_t e = ofdm::launch_soft_demap_csi(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "soft demap csi launch");
    return OFDM_OK;
}

int ofdm_rx_demod_soft(ofdm_ctx* c, const double* iq, const int16_t* iq16, size_t nframes, size_t frame_stride,
                       const double* chan, size_t chan_stride, double scale, const double* frame_scale, int fmt,
                       void* llr_out, double* constell_out, uint8_t* bytes_out, const uint8_t* ref_bytes,
                       unsigned long long* bit_errors, void* stream)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null argument");
    if ((iq == nullptr) == (iq16 == nullptr)) return fail(OFDM_ERR_INVALID, "exactly one of iq, iq16");
    if (int rc = soft_args_check(c, scale, fmt, llr_out)) return rc;
    if (frame_scale && ((uintptr_t)frame_scale & 7)) return fail(OFDM_ERR_INVALID, "frame_scale must be 8-byte aligned");
    ofdm::SoftArgs sa{llr_out, frame_scale, scale, fmt};
    return rx_demod_impl(c, iq, iq16, nframes, frame_stride, chan, chan_stride, constell_out, bytes_out, ref_bytes,
                         bit_errors, stream, nullptr, &sa);
}

// ---- channel code
int ofdm_fec_coded_bits(size_t info_bits, int rate, size_t* coded_bits)
{
    if (!coded_bits) return fail(OFDM_ERR_INVALID, "null argument");
    if (!fec_rate_ok(rate)) return fail(OFDM_ERR_INVALID, "rate is not OFDM_FEC_R12 / R23 / R34");
    if (info_bits == 0 || info_bits > SIZE_MAX / 4) return fail(OFDM_ERR_INVALID, "info_bits out of range");
    *coded_bits = fec_coded(info_bits, rate);
    return OFDM_OK;
}

int ofdm_fec_max_info_bits(size_t capacity_bits, int rate, size_t* info_bits)
{
    if (!info_bits) return fail(OFDM_ERR_INVALID, "null argument");
    if (!fec_rate_ok(rate)) return fail(OFDM_ERR_INVALID, "rate is not OFDM_FEC_R12 / R23 / R34");
    if (capacity_bits > SIZE_MAX / 4) return fail(OFDM_ERR_INVALID, "capacity_bits out of range");
    if (fec_coded(1, rate) > capacity_bits) return fail(OFDM_ERR_INVALID, "no codeword fits %zu bits", capacity_bits);
    size_t lo = 1, hi = capacity_bits;  // coded_bits grows with info_bits and exceeds it: the answer is in [lo, hi]
    while (lo < hi) {
        const size_t mid = lo + (hi - lo + 1) / 2;
        if (fec_coded(mid, rate) <= capacity_bits) lo = mid;
        else hi = mid - 1;
    }
    *info_bits = lo;
    return OFDM_OK;
}

int ofdm_fec_workspace_size(size_t ncw, size_t info_bits, size_t* bytes)
{
    if (!bytes) return fail(OFDM_ERR_INVALID, "null argument");
    if (info_bits == 0 || info_bits > (size_t)ofdm::FEC_MAX_INFO_BITS)
        return fail(OFDM_ERR_INVALID, "info_bits must be in [1, 2^20]");
    const size_t words = (size_t)ofdm::fec_steps_padded((long)info_bits);
    if (words <= (size_t)ofdm::FEC_LDS_STEPS) {
        *bytes = 0;
        return OFDM_OK;
    }
    if (ncw > SIZE_MAX / (words * 8)) return fail(OFDM_ERR_INVALID, "ncw out of range");
    *bytes = ncw * words * 8;
    return OFDM_OK;
}

int ofdm_fec_encode(ofdm_ctx* c, const uint8_t* info, size_t info_stride, size_t ncw, size_t info_bits, int rate,
                    uint8_t* coded, size_t coded_stride, void* stream)
{
    if (!c || !info || !coded) return fail(OFDM_ERR_INVALID, "null argument");
    if (!fec_rate_ok(rate)) return fail(OFDM_ERR_INVALID, "rate is not OFDM_FEC_R12 / R23 / R34");
    if (info_bits == 0 || info_bits > (size_t)ofdm::FEC_MAX_INFO_BITS)
        return fail(OFDM_ERR_INVALID, "info_bits must be in [1, 2^20]");
    const size_t cb = fec_coded(info_bits, rate);
    if (info_stride < (info_bits + 7) / 8) return fail(OFDM_ERR_INVALID, "info_stride below ceil(info_bits/8)");
    if (coded_stride < (cb + 7) / 8) return fail(OFDM_ERR_INVALID, "coded_stride below ceil(coded_bits/8)");
    if (ncw > (size_t)LONG_MAX / std::max(info_stride, coded_stride)) return fail(OFDM_ERR_INVALID, "ncw out of range");
    if (ncw == 0) return OFDM_OK;
    ofdm::FecEncArgs a{info, coded, (long)info_stride, (long)coded_stride, (long)ncw, (long)info_bits, (long)cb, rate};
    hipError_t e = ofdm::launch_fec_encode(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "fec encode launch");
    return OFDM_OK;
}

int ofdm_fec_decode(ofdm_ctx* c, const void* llr, int fmt, size_t llr_stride, size_t ncw, size_t info_bits, int rate,
                    void* workspace, size_t workspace_bytes, uint8_t* info_out, size_t info_stride,
                    const uint8_t* ref_info, unsigned long long* bit_errors, void* stream)
{
    if (!c || !llr || !info_out) return fail(OFDM_ERR_INVALID, "null argument");
    if (!fec_rate_ok(rate)) return fail(OFDM_ERR_INVALID, "rate is not OFDM_FEC_R12 / R23 / R34");
    if (fmt != OFDM_LLR_F32 && fmt != OFDM_LLR_I8) return fail(OFDM_ERR_INVALID, "fmt is not OFDM_LLR_F32 / OFDM_LLR_I8");
    if (info_bits == 0 || info_bits > (size_t)ofdm::FEC_MAX_INFO_BITS)
        return fail(OFDM_ERR_INVALID, "info_bits must be in [1, 2^20]");
    if (fmt == OFDM_LLR_F32 && ((uintptr_t)llr & 3)) return fail(OFDM_ERR_INVALID, "F32 llr must be 4-byte aligned");
    if (bit_errors && ((uintptr_t)bit_errors & 7)) return fail(OFDM_ERR_INVALID, "bit_errors must be 8-byte aligned");
    if (llr_stride < fec_coded(info_bits, rate)) return fail(OFDM_ERR_INVALID, "llr_stride below coded_bits");
    if (info_stride < (info_bits + 7) / 8) return fail(OFDM_ERR_INVALID, "info_stride below ceil(info_bits/8)");
    if (ncw > (size_t)LONG_MAX / 4 / std::max(info_stride, llr_stride)) return fail(OFDM_ERR_INVALID, "ncw out of range");
    size_t need = 0;
    if (int rc = ofdm_fec_workspace_size(ncw, info_bits, &need)) return rc;
    if (need) {
        if (!workspace) return fail(OFDM_ERR_INVALID, "this length needs a workspace (ofdm_fec_workspace_size)");
        if (!aligned16(workspace)) return fail(OFDM_ERR_INVALID, "workspace must be 16-byte aligned");
        if (workspace_bytes < need) return fail(OFDM_ERR_INVALID, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    }
    if (ncw == 0) return OFDM_OK;
    ofdm::FecDecArgs a{};
    a.llr = llr;
    a.llr_stride = (long)llr_stride;
    a.ncw = (long)ncw;
    a.info_bits = (long)info_bits;
    a.ws = need ? static_cast<unsigned long long*>(workspace) : nullptr;
    a.out = info_out;
    a.ref = ref_info;
    a.bit_errors = bit_errors;
    a.info_stride = (long)info_stride;
    a.fmt = fmt;
    a.rate = rate;
    // OFDM_FEC_GATHER=lds: the other predecessor-gather variant (A/B measurements, tools/coded_ber.py)
    const char* g = getenv("OFDM_FEC_GATHER");
    a.gather = g && !strcmp(g, "lds") ? 1 : 0;
    hipError_t e = ofdm::launch_fec_decode(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "fec decode launch");
    return OFDM_OK;
}

// ---- interleaver and scrambler
int ofdm_interleave_default(const ofdm_ctx* c, size_t* block_bits, size_t* cols, size_t* s)
{
    if (!c || !block_bits || !cols || !s) return fail(OFDM_ERR_INVALID, "null argument");
    const size_t n = (size_t)c->D * (size_t)c->k, rot = c->k >= 2 ? (size_t)c->k / 2 : 1;
    if (!il_params_ok(n, 16, rot))
        return fail(OFDM_ERR_UNSUPPORTED, "num_data_subc*modType = %zu bits is no valid block of 16 columns", n);
    *block_bits = n;
    *cols = 16;
    *s = rot;
    return OFDM_OK;
}

int ofdm_interleave_bits(ofdm_ctx* c, const uint8_t* in, size_t nblocks, size_t block_bits, size_t cols, size_t s,
                         int dir, uint8_t* out, void* stream)
{
    return interleave_impl(c, in, ofdm::IL_BITS, nblocks, block_bits, cols, s, dir, out, stream);
}

int ofdm_interleave_llr(ofdm_ctx* c, const void* in, int fmt, size_t nblocks, size_t block_bits, size_t cols,
                        size_t s, int dir, void* out, void* stream)
{
    if (fmt != OFDM_LLR_F32 && fmt != OFDM_LLR_I8) return fail(OFDM_ERR_INVALID, "fmt is not OFDM_LLR_F32 / OFDM_LLR_I8");
    return interleave_impl(c, in, fmt == OFDM_LLR_F32 ? ofdm::IL_F32 : ofdm::IL_I8, nblocks, block_bits, cols, s, dir,
                           out, stream);
}

int ofdm_scramble(ofdm_ctx* c, const uint8_t* in, size_t in_stride, size_t ncw, size_t nbits, unsigned seed,
                  const uint8_t* seeds, uint8_t* out, size_t out_stride, void* stream)
{
    if (!c || !in || !out) return fail(OFDM_ERR_INVALID, "null argument");
    if (nbits == 0 || nbits > (size_t)LONG_MAX / 2) return fail(OFDM_ERR_INVALID, "nbits out of range");
    const size_t nbytes = (nbits + 7) / 8;
    if (in_stride < nbytes || out_stride < nbytes) return fail(OFDM_ERR_INVALID, "stride below ceil(nbits/8)");
    if (!seeds && (seed < 1 || seed > 127)) return fail(OFDM_ERR_INVALID, "seed %u is not in 1..127", seed);
    if (in == out && in_stride != out_stride) return fail(OFDM_ERR_INVALID, "in place needs equal strides");
    if (ncw > (size_t)LONG_MAX / std::max(in_stride, out_stride)) return fail(OFDM_ERR_INVALID, "ncw out of range");
    if (ncw == 0) return OFDM_OK;
    ofdm::ScrArgs a{in, out, seeds, (long)in_stride, (long)out_stride, (long)ncw, (long)nbits, seed};
    hipError_t e = ofdm::launch_scramble(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "scramble launch");
    return OFDM_OK;
}

// ---- MAC framing and frame check
// The argument rules the two batched calls share; *cap receives the payload capacity.
static int mac_sizes_check(size_t frame_len, int fcs, size_t frame_stride, size_t nframes, size_t* cap)
{
    if (fcs != OFDM_FCS_NONE && fcs != OFDM_FCS_CRC32) return fail(OFDM_ERR_INVALID, "fcs is not OFDM_FCS_NONE / OFDM_FCS_CRC32");
    const size_t f = fcs == OFDM_FCS_CRC32 ? 4 : 0;
    if (frame_len < ofdm::MAC_HDR + f || frame_len > ofdm::MAC_MAX_FRAME)
        return fail(OFDM_ERR_INVALID, "frame_len %zu is not in [%zu, %u]", frame_len, ofdm::MAC_HDR + f, ofdm::MAC_MAX_FRAME);
    if (frame_stride < frame_len) return fail(OFDM_ERR_INVALID, "frame_stride below frame_len");
    if (nframes > (size_t)LONG_MAX / frame_stride) return fail(OFDM_ERR_INVALID, "nframes out of range");
    *cap = frame_len - ofdm::MAC_HDR - f;
    return OFDM_OK;
}

static bool mac_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

int ofdm_mac_payload_len(size_t frame_len, int fcs, size_t* cap)
{
    if (!cap) return fail(OFDM_ERR_INVALID, "null argument");
    size_t v = 0;
    if (int rc = mac_sizes_check(frame_len, fcs, frame_len, 1, &v)) return rc;
    *cap = v;
    return OFDM_OK;
}

// (the context is asked for last: the argument rules hold without a device)
int ofdm_mac_write(ofdm_ctx* c, const uint8_t* payload, size_t payload_stride, size_t payload_len, size_t nframes,
                   size_t frame_len, int fcs, unsigned tx_id, unsigned rx_id, unsigned seq0, const uint16_t* seqs,
                   uint8_t* frames_out, size_t frame_stride, void* stream)
{
    size_t cap = 0;
    if (int rc = mac_sizes_check(frame_len, fcs, frame_stride, nframes, &cap)) return rc;
    if (payload_len > cap) return fail(OFDM_ERR_INVALID, "payload_len %zu above the frame's %zu", payload_len, cap);
    if (payload_stride < payload_len) return fail(OFDM_ERR_INVALID, "payload_stride below payload_len");
    if (payload_stride && nframes > (size_t)LONG_MAX / payload_stride) return fail(OFDM_ERR_INVALID, "nframes out of range");
    if (tx_id > 65535 || rx_id > 65535 || seq0 > 65535) return fail(OFDM_ERR_INVALID, "tx_id, rx_id and seq0 are 16-bit values");
    if (seqs && ((uintptr_t)seqs & 1)) return fail(OFDM_ERR_INVALID, "seqs must be 2-byte aligned");
    if (!frames_out || (!payload && payload_len)) return fail(OFDM_ERR_INVALID, "null argument");
    if (nframes && mac_overlap(payload, (nframes - 1) * payload_stride + payload_len, frames_out, nframes * frame_stride))
        return fail(OFDM_ERR_INVALID, "payload and frames_out overlap");
    if (!c) return fail(OFDM_ERR_INVALID, "null context");
    if (nframes == 0) return OFDM_OK;
    ofdm::MacWriteArgs a{};
    a.payload = payload;
    a.frames = frames_out;
    a.seqs = seqs;
    a.payload_stride = payload_stride;
    a.frame_stride = frame_stride;
    a.nframes = nframes;
    a.payload_len = (unsigned)payload_len;
    a.frame_len = (unsigned)frame_len;
    a.m = (unsigned)(cap + ofdm::MAC_HDR);
    a.tx_id = tx_id;
    a.rx_id = rx_id;
    a.seq0 = seq0;
    hipError_t e = ofdm::launch_mac_write(a, fcs == OFDM_FCS_CRC32, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "mac write launch");
    return OFDM_OK;
}

int ofdm_mac_read(ofdm_ctx* c, const uint8_t* frames, size_t frame_stride, size_t nframes, size_t frame_len, int fcs,
                  int expect_rx_id, uint8_t* payload_out, size_t payload_stride, ofdm_mac_info* info_out,
                  unsigned long long* frame_errors, void* stream)
{
    size_t cap = 0;
    if (int rc = mac_sizes_check(frame_len, fcs, frame_stride, nframes, &cap)) return rc;
    if (expect_rx_id > 65535) return fail(OFDM_ERR_INVALID, "expect_rx_id is a 16-bit value, or negative for any");
    if (payload_out && payload_stride < cap) return fail(OFDM_ERR_INVALID, "payload_stride below the frame's %zu payload bytes", cap);
    if (payload_out && payload_stride && nframes > (size_t)LONG_MAX / payload_stride)
        return fail(OFDM_ERR_INVALID, "nframes out of range");
    if (info_out && !aligned16(info_out)) return fail(OFDM_ERR_INVALID, "info_out must be 16-byte aligned");
    if (frame_errors && ((uintptr_t)frame_errors & 7)) return fail(OFDM_ERR_INVALID, "frame_errors must be 8-byte aligned");
    if (!frames || (!payload_out && !info_out && !frame_errors)) return fail(OFDM_ERR_INVALID, "null argument");
    if (nframes) {
        const size_t in_bytes = (nframes - 1) * frame_stride + frame_len;
        if ((payload_out && mac_overlap(frames, in_bytes, payload_out, (nframes - 1) * payload_stride + cap)) ||
            (info_out && mac_overlap(frames, in_bytes, info_out, nframes * sizeof(ofdm_mac_info))) ||
            (frame_errors && mac_overlap(frames, in_bytes, frame_errors, 8)))
            return fail(OFDM_ERR_INVALID, "frames and an output overlap");
    }
    if (!c) return fail(OFDM_ERR_INVALID, "null context");
    if (nframes == 0) return OFDM_OK;
    ofdm::MacReadArgs a{};
    a.frames = frames;
    a.payload = payload_out;
    a.info = reinterpret_cast<ofdm::MacU4*>(info_out);
    a.frame_errors = frame_errors;
    a.frame_stride = frame_stride;
    a.payload_stride = payload_out ? payload_stride : 0;
    a.nframes = nframes;
    a.frame_len = (unsigned)frame_len;
    a.m = (unsigned)(cap + ofdm::MAC_HDR);
    a.expect_rx_id = expect_rx_id;
    hipError_t e = ofdm::launch_mac_read(a, fcs == OFDM_FCS_CRC32, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "mac read launch");
    return OFDM_OK;
}

int ofdm_map(ofdm_ctx* c, const uint8_t* bytes, size_t nbytes, double* points_out, void* stream)
{
    if (!c || !bytes || !points_out) return fail(OFDM_ERR_INVALID, "null argument");
    hipError_t e = ofdm::launch_map(bytes, (long)nbytes, c->k, c->d_const, reinterpret_cast<double2*>(points_out),
                                    (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "map launch");
    return OFDM_OK;
}

int ofdm_fft_write(ofdm_ctx* c, const double* points, size_t nframes, double* fft_buf, void* stream)
{
    if (!c || !points || !fft_buf) return fail(OFDM_ERR_INVALID, "null argument");
    if (!aligned16(points) || !aligned16(fft_buf)) return fail(OFDM_ERR_INVALID, "buffers must be 16-byte aligned");
    if (nframes == 0) return OFDM_OK;
    ofdm::TxArgs a{};
    fill_tx(c, a, nullptr, nframes, fft_buf, (size_t)c->N * c->S, nullptr, nullptr);
    a.points = reinterpret_cast<const double2*>(points);
    a.cp = 0;  // FFT_buf holds bodies only
    hipError_t e = ofdm::launch_tx(c->logn, a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "fft_write launch");
    return OFDM_OK;
}

int ofdm_fft_read(ofdm_ctx* c, const double* fft_buf, size_t nframes, double* restored, void* stream)
{
    if (!c || !fft_buf || !restored) return fail(OFDM_ERR_INVALID, "null argument");
    if (!aligned16(fft_buf) || !aligned16(restored)) return fail(OFDM_ERR_INVALID, "buffers must be 16-byte aligned");
    if (nframes == 0) return OFDM_OK;
    ofdm::RxArgs a{};
    a.tab = c->tables(false);
    a.iq = reinterpret_cast<const double2*>(fft_buf);
    a.nframes = (long)nframes;
    a.frame_stride = (long)c->N * c->S;
    a.constell = reinterpret_cast<double2*>(restored);
    a.S = c->S;
    a.D = c->D;
    a.P = c->P;
    a.seg = c->seg;
    a.cp = 0;  // no CP in FFT_buf
    a.k = c->k;
    a.bytes_per_frame = c->geo.bytes_per_frame;
    a.pilot_ampl = (double)c->p.pilot_ampl / 1000;
    a.queue = rx_queue(c, (hipStream_t)stream);
    if (!(c->S <= ofdm::RX_SMAX && c->D <= ofdm::RX_DPT * (c->N / 8))) a.ystage = a.constell;
    hipError_t e = ofdm::launch_rx(c->logn, a, (hipStream_t)stream, nullptr);
    if (e != hipSuccess) {
        rx_queue_reset(c, a.queue, (hipStream_t)stream);
        return hip_fail(e, "fft_read launch");
    }
    return OFDM_OK;
}

int ofdm_bit_convert(ofdm_ctx* c, const uint8_t* in, size_t len, int in_bits, int out_bits, uint8_t* out,
                     size_t* out_len, void* stream)
{
    if (!c || (len && (!in || !out))) return fail(OFDM_ERR_INVALID, "null argument");
    if (in_bits < 1 || in_bits > 8 || out_bits < 1 || out_bits > 8) return fail(OFDM_ERR_INVALID, "bits must be 1..8");
    const size_t total = len * (size_t)in_bits;
    const size_t n = total / out_bits + (total % out_bits > 0);
    if (out_len) *out_len = n;
    hipError_t e = ofdm::launch_bit_convert(in, (long)len, in_bits, out_bits, out, (long)n, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "bit_convert launch");
    return OFDM_OK;
}

int ofdm_int16_to_double(ofdm_ctx* c, const int16_t* in, size_t n, double* out, void* stream)
{
    if (!c || (n && (!in || !out))) return fail(OFDM_ERR_INVALID, "null argument");
    if (((uintptr_t)in & 3) || !aligned16(out)) return fail(OFDM_ERR_INVALID, "misaligned buffers");
    hipError_t e = ofdm::launch_i16_to_f64(in, (long)n, out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "int16_to_double launch");
    return OFDM_OK;
}

int ofdm_double_to_int16(ofdm_ctx* c, const double* in, size_t n, int16_t* out, void* stream)
{
    if (!c || (n && (!in || !out))) return fail(OFDM_ERR_INVALID, "null argument");
    if (!aligned16(in) || ((uintptr_t)out & 3)) return fail(OFDM_ERR_INVALID, "misaligned buffers");
    hipError_t e = ofdm::launch_f64_to_i16(in, (long)n, (double)c->p.mult, out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "double_to_int16 launch");
    return OFDM_OK;
}

// ---- sync front end (ofdm_sync.hip)
int ofdm_t2_scan(ofdm_ctx* c, const double* iq, size_t n, long start, double* rel_out, int* first_out, void* stream)
{
    if (!c || !iq) return fail(OFDM_ERR_INVALID, "null argument");
    if (c->t2_logn < 0) return fail(OFDM_ERR_UNSUPPORTED, "T2 detector needs T2sin_size = 2^a, 64..4096");
    if (start < 0) return fail(OFDM_ERR_INVALID, "start < 0");
    if (!aligned16(iq)) return fail(OFDM_ERR_INVALID, "iq must be 16-byte aligned");
    ofdm::T2Args a{};
    a.iq = reinterpret_cast<const double2*>(iq);
    a.tw = c->d_t2tw;
    a.start = start;
    a.nblocks = (long)n > start ? ((long)n - start) / c->t2 : 0;
    const int sm = (int)c->p.smooth, f1 = (int)c->p.t2_sin_f1, f2 = (int)c->p.t2_sin_f2;
    a.a1 = std::max(0, f1 - sm);
    a.b1 = std::min(c->t2 - 1, f1 + sm);
    a.a2 = std::max(0, f2 - sm);
    a.b2 = std::min(c->t2 - 1, f2 + sm);
    a.level = (double)c->p.t2_sin_level / 1000;
    a.rel_out = rel_out;
    a.first_scratch = c->d_first;
    hipError_t e = ofdm::launch_t2_scan(c->t2_logn, a, first_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "t2_scan launch");
    return OFDM_OK;
}

// The launch arguments of find_preamble / preamble_corr for `nstarts` start
// indices: the context's template and lags, and its split scratch when the
// call fits it (else the one-workgroup form: hv_scratch stays null).
static ofdm::PreambleArgs preamble_args(ofdm_ctx* c, const double* iq, size_t n, const int* starts, size_t nstarts)
{
    ofdm::PreambleArgs a{};
    a.iq = reinterpret_cast<const double2*>(iq);
    a.n = (long)n;
    a.starts = starts;
    a.nstarts = (long)nstarts;
    a.templ = c->d_templ;
    a.L = (int)c->p.pr_sin_len;
    a.cycles = (int)(2 * c->p.t2sin_size + c->p.pr_sin_len);
    a.level = (double)c->p.pr_level / 1000;
    if (nstarts <= ofdm_ctx::PRE_SCRATCH_STARTS) {
        a.hv_scratch = c->d_pre_hv;
        a.done = c->d_pre_done;
    }
    return a;
}

// What launch_find_preamble would refuse, as status codes of the header,
// before anything is issued: more start indices than one launch takes, and a
// T2sin_size / pr_sin_len whose lags do not fit one workgroup's LDS (the
// launcher's own arithmetic on the same arguments).
static int preamble_fits(ofdm_ctx* c, const ofdm::PreambleArgs& a)
{
    if (a.nstarts > ofdm::FIND_PREAMBLE_MAX_STARTS)
        return fail(OFDM_ERR_INVALID, "find_preamble: nstarts=%ld exceeds %ld per call", a.nstarts,
                    ofdm::FIND_PREAMBLE_MAX_STARTS);
    const size_t need = ofdm::find_preamble_lds(a);
    if (need > ofdm::FIND_PREAMBLE_MAX_LDS)
        return fail(OFDM_ERR_UNSUPPORTED, "find_preamble: T2sin_size=%ld with pr_sin_len=%ld needs %zu bytes of LDS "
                                          "(limit %zu)", c->p.t2sin_size, c->p.pr_sin_len, need,
                    ofdm::FIND_PREAMBLE_MAX_LDS);
    return OFDM_OK;
}

int ofdm_find_preamble(ofdm_ctx* c, const double* iq, size_t n, const int* starts, size_t nstarts, int* idx_out,
                       void* stream)
{
    if (!c || !iq || (nstarts && (!starts || !idx_out))) return fail(OFDM_ERR_INVALID, "null argument");
    if (!aligned16(iq)) return fail(OFDM_ERR_INVALID, "iq must be 16-byte aligned");
    if (nstarts == 0) return OFDM_OK;
    if (nstarts > (size_t)LONG_MAX) return fail(OFDM_ERR_INVALID, "find_preamble: nstarts out of range");
    ofdm::PreambleArgs a = preamble_args(c, iq, n, starts, nstarts);
    a.idx_out = idx_out;
    if (int rc = preamble_fits(c, a)) return rc;
    hipError_t e = ofdm::launch_find_preamble(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "find_preamble launch");
    return OFDM_OK;
}

int ofdm_preamble_corr(ofdm_ctx* c, const double* iq, size_t n, long start, double* cor_out, void* stream)
{
    if (!c || !iq || !cor_out) return fail(OFDM_ERR_INVALID, "null argument");
    if (!aligned16(iq)) return fail(OFDM_ERR_INVALID, "iq must be 16-byte aligned");
    if (start < INT32_MIN || start > INT32_MAX) return fail(OFDM_ERR_INVALID, "start out of range");
    int* d_start = c->d_first + 2;  // scratch word 2: the one start index
    ofdm::PreambleArgs a = preamble_args(c, iq, n, d_start, 1);
    a.cor_out = cor_out;
    if (int rc = preamble_fits(c, a)) return rc;
    if (capturing((hipStream_t)stream))
        return capture_refused("ofdm_preamble_corr (it stages `start` from the host and synchronises)");
    const int s32 = (int)start;
    HIP_TRY(hipMemcpyAsync(d_start, &s32, sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream));
    hipError_t e = ofdm::launch_find_preamble(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "preamble_corr launch");
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the start word is host-staged
    return OFDM_OK;
}

int ofdm_cfo_estimate(ofdm_ctx* c, const double* x, size_t nframes, size_t stride, int nsym, double* cfo_out,
                      void* stream)
{
    if (!c || !x || !cfo_out) return fail(OFDM_ERR_INVALID, "null argument");
    if (nsym < 1 || stride < (size_t)c->L * nsym) return fail(OFDM_ERR_INVALID, "bad nsym / frame_stride");
    if (!aligned16(x)) return fail(OFDM_ERR_INVALID, "x must be 16-byte aligned");
    if (nframes == 0) return OFDM_OK;
    ofdm_ctx::CfoPlan* pl = nullptr;
    int rc = cfo_plan(c, nsym, &pl, (hipStream_t)stream);
    if (rc) return rc;
    ofdm::CfoArgs a{};
    a.x = reinterpret_cast<const double2*>(x);
    a.nframes = (long)nframes;
    a.frame_stride = (long)stride;
    a.tw_sub = pl->tw_sub;
    a.tw_full = pl->tw_full;
    a.borders = pl->borders;
    a.P = c->P;
    a.cfo_out = cfo_out;
    a.host_out = 1;  // the public entry: cfo_out may be pinned host memory (header)
    hipError_t e = ofdm::launch_cfo(pl->logm, pl->g, a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "cfo launch");
    return OFDM_OK;
}

int ofdm_freq_shift(ofdm_ctx* c, double* x, size_t nframes, size_t stride, size_t nsamples, const double* cfo,
                    void* stream)
{
    if (!c || !x || !cfo) return fail(OFDM_ERR_INVALID, "null argument");
    if (nframes > 1 && stride < nsamples) return fail(OFDM_ERR_INVALID, "frame_stride < nsamples");
    if (!aligned16(x)) return fail(OFDM_ERR_INVALID, "x must be 16-byte aligned");
    ofdm::ShiftArgs a{reinterpret_cast<double2*>(x), (long)nframes, (long)stride, (long)nsamples, cfo};
    hipError_t e = ofdm::launch_freq_shift(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "freq_shift launch");
    return OFDM_OK;
}

int ofdm_cp_sync(ofdm_ctx* c, double* x, size_t nframes, size_t stride, int nsym, void* stream)
{
    if (!c || !x) return fail(OFDM_ERR_INVALID, "null argument");
    if (nsym < 1 || nsym > 64 || (nframes > 1 && stride < (size_t)c->L * nsym))
        return fail(OFDM_ERR_INVALID, "bad nsym / frame_stride");
    if (!aligned16(x)) return fail(OFDM_ERR_INVALID, "x must be 16-byte aligned");
    ofdm::CpArgs a{reinterpret_cast<double2*>(x), (long)nframes, (long)stride, nsym, c->N, c->cp};
    hipError_t e = ofdm::launch_cp_sync(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "cp_sync launch");
    return OFDM_OK;
}

int ofdm_phase_sync(ofdm_ctx* c, double* x, size_t nframes, size_t stride, size_t nsamples, const double* pr,
                    size_t pr_len, void* stream)
{
    if (!c || !x) return fail(OFDM_ERR_INVALID, "null argument");
    if (!pr) {
        pr = reinterpret_cast<const double*>(c->d_preamble.get());
        pr_len = (size_t)c->geo.preamble_len;
    }
    if (pr_len > nsamples && nframes > 1 && stride < pr_len) return fail(OFDM_ERR_INVALID, "pr_len exceeds the form");
    if (!aligned16(x) || !aligned16(pr)) return fail(OFDM_ERR_INVALID, "buffers must be 16-byte aligned");
    ofdm::PhaseArgs a{reinterpret_cast<double2*>(x), (long)nframes, (long)stride, (long)nsamples,
                      reinterpret_cast<const double2*>(pr), (long)pr_len};
    hipError_t e = ofdm::launch_phase_sync(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "phase_sync launch");
    return OFDM_OK;
}

int ofdm_sync_chain(ofdm_ctx* c, double* x, size_t nframes, size_t stride, size_t nsamples, int nsym,
                    const double* cfo, double* shift_out, double* cp_out, double* phase_out, size_t out_stride,
                    void* stream)
{
    if (!c || !x || !cfo) return fail(OFDM_ERR_INVALID, "null argument");
    if (nsym < 1 || nsym > 64 || (size_t)c->L * nsym > nsamples) return fail(OFDM_ERR_INVALID, "bad nsym / nsamples");
    if (nframes > 1 && stride < nsamples) return fail(OFDM_ERR_INVALID, "frame_stride < nsamples");
    if ((size_t)c->geo.preamble_len > nsamples) return fail(OFDM_ERR_INVALID, "the preamble exceeds the form");
    double* outs[3] = {shift_out, cp_out, phase_out};
    for (double* o : outs)
        if (o && nframes > 1 && out_stride < nsamples) return fail(OFDM_ERR_INVALID, "out_stride < nsamples");
    if (!aligned16(x) || !aligned16(shift_out) || !aligned16(cp_out) || !aligned16(phase_out))
        return fail(OFDM_ERR_INVALID, "buffers must be 16-byte aligned");
    if (nframes == 0 || nsamples == 0) return OFDM_OK;
    ofdm::SyncChainArgs a{};
    a.x = reinterpret_cast<double2*>(x);
    a.nframes = (long)nframes;
    a.frame_stride = (long)stride;
    a.nsamples = (long)nsamples;
    a.cfo = cfo;
    a.nsym = nsym;
    a.N = c->N;
    a.cp = c->cp;
    a.pr = c->d_preamble;
    a.pr_len = (long)c->geo.preamble_len;
    for (int k = 0; k < 3; ++k) a.out[k] = reinterpret_cast<double2*>(outs[k]);
    a.out_stride = (long)out_stride;
    hipError_t e = ofdm::launch_sync_chain(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "sync_chain launch");
    return OFDM_OK;
}

int ofdm_chan_estimate(ofdm_ctx* c, const double* x, size_t nframes, size_t stride, double* chan_out,
                       size_t chan_stride, void* stream)
{
    if (!c || !x || !chan_out) return fail(OFDM_ERR_INVALID, "null argument");
    if (!aligned16(x) || !aligned16(chan_out)) return fail(OFDM_ERR_INVALID, "buffers must be 16-byte aligned");
    if (c->P > c->N / 8) return fail(OFDM_ERR_UNSUPPORTED, "num_pilot_subc > fft_size/8");
    ofdm::ChanArgs a{};
    a.tab = c->tables(true);
    a.x = reinterpret_cast<const double2*>(x);
    a.nframes = (long)nframes;
    a.frame_stride = (long)stride;
    a.mod_pre = c->d_modpre;
    a.chan_out = reinterpret_cast<double2*>(chan_out);
    a.chan_stride = (long)chan_stride;
    a.npr = c->npr;
    a.D = c->D;
    a.P = c->P;
    a.cp = c->cp;
    a.pilot_ampl = (double)c->p.pilot_ampl / 1000;
    hipError_t e = ofdm::launch_chan(c->logn, a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "chan launch");
    return OFDM_OK;
}

int ofdm_chan_estimate_ls(ofdm_ctx* c, const double* x, size_t nframes, size_t stride, int smooth, double* chan_out,
                          size_t chan_stride, double* csi_out, size_t csi_stride, void* stream)
{
    if (!c || !x) return fail(OFDM_ERR_INVALID, "null argument");
    if (!chan_out && !csi_out) return fail(OFDM_ERR_INVALID, "chan_out and csi_out are both null");
    if (smooth < 0 || smooth > ofdm::CSI_SMOOTH_MAX) return fail(OFDM_ERR_INVALID, "smooth outside 0..64");
    if ((chan_out && chan_stride < (size_t)c->D) || (csi_out && csi_stride < (size_t)c->D))
        return fail(OFDM_ERR_INVALID, "output stride < num_data_subc");
    if (!aligned16(x) || !aligned16(chan_out)) return fail(OFDM_ERR_INVALID, "complex buffers must be 16-byte aligned");
    if ((uintptr_t)csi_out & 7) return fail(OFDM_ERR_INVALID, "csi_out must be 8-byte aligned");
    if (nframes > 0x7fffffffu) return fail(OFDM_ERR_INVALID, "nframes out of range");
    if (c->P > c->N / 8) return fail(OFDM_ERR_UNSUPPORTED, "num_pilot_subc > fft_size/8");
    if (ofdm::chan_ls_lds_bytes(c->logn, c->npr, c->D, c->P) > ofdm::CSI_LDS_MAX)
        return fail(OFDM_ERR_UNSUPPORTED, "the preamble form's pilots and carriers do not fit the LDS");
    if (nframes == 0) return OFDM_OK;
    ofdm::ChanLsArgs a{};
    a.tab = c->tables(true);
    a.x = reinterpret_cast<const double2*>(x);
    a.nframes = (long)nframes;
    a.frame_stride = (long)stride;
    a.mod_pre = c->d_modpre;
    a.chan_out = reinterpret_cast<double2*>(chan_out);
    a.csi_out = csi_out;
    a.chan_stride = (long)chan_stride;
    a.csi_stride = (long)csi_stride;
    a.npr = c->npr;
    a.D = c->D;
    a.P = c->P;
    a.cp = c->cp;
    a.smooth = smooth;
    a.pilot_ampl = (double)c->p.pilot_ampl / 1000;
    hipError_t e = ofdm::launch_chan_ls(c->logn, a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "chan_ls launch");
    return OFDM_OK;
}

int ofdm_sync_frames(ofdm_ctx* c, double* frames, size_t nframes, size_t stride, int stages, const double* cfo_in,
                     double* cfo_out, double* chan_out, void* stream)
{
    if (!c || !frames) return fail(OFDM_ERR_INVALID, "null argument");
    const int nsym = c->npr + c->S;
    const size_t nsamples = (size_t)c->L * nsym;
    if (nframes > 1 && stride < nsamples) return fail(OFDM_ERR_INVALID, "frame_stride < preamble+message");
    if (nframes == 0) return OFDM_OK;
    const double* cfo = cfo_in;
    int rc;
    if (stages & OFDM_SYNC_CFO) {
        double* dst = cfo_out;
        if (!dst) {
            const size_t need = nframes * sizeof(double);
            if (need > c->d_cfo_scratch.bytes && capturing((hipStream_t)stream))
                return capture_refused("growing the CFO scratch (cfo_out = NULL)");
            if ((rc = grow(c, c->d_cfo_scratch, need))) return rc;
            dst = static_cast<double*>(c->d_cfo_scratch.p.get());
        }
        if ((rc = ofdm_cfo_estimate(c, frames, nframes, stride, c->npr, dst, stream))) return rc;
        cfo = dst;
    }
    if (stages & OFDM_SYNC_FREQ_SHIFT) {
        if (!cfo) return fail(OFDM_ERR_INVALID, "freq shift without a CFO (set OFDM_SYNC_CFO or pass cfo_in)");
        if ((rc = ofdm_freq_shift(c, frames, nframes, stride, nsamples, cfo, stream))) return rc;
    }
    if ((stages & OFDM_SYNC_CP) && (rc = ofdm_cp_sync(c, frames, nframes, stride, nsym, stream))) return rc;
    if ((stages & OFDM_SYNC_PHASE) && (rc = ofdm_phase_sync(c, frames, nframes, stride, nsamples, nullptr, 0, stream)))
        return rc;
    if ((stages & OFDM_SYNC_CHAN) && chan_out &&
        (rc = ofdm_chan_estimate(c, frames, nframes, stride, chan_out, (size_t)c->D, stream)))
        return rc;
    return OFDM_OK;
}

// The stream receiver (ofdm_stream_call.cpp). ofdm_rx_stream / _i16: the whole
// stream from rx.cpp's initial state, no shard report.
int ofdm_rx_stream(ofdm_ctx* c, const double* iq, size_t n, size_t max_frames, long chunk, long* pb_out,
                   uint8_t* bytes_out, double* constell_out, double* cfo_out, size_t* nframes_out, void* stream)
{
    if (!c || !iq) return fail(OFDM_ERR_INVALID, "null argument");
    const ofdm::StreamCall a{iq, nullptr, n, max_frames, chunk, pb_out, bytes_out, constell_out, cfo_out, nframes_out,
                             stream, initial_state(c), 0, (long)n, nullptr, nullptr, 0, nullptr, nullptr};
    return ofdm::rx_stream_call(c, a);
}

int ofdm_rx_stream_i16(ofdm_ctx* c, const int16_t* iq16, size_t n, size_t max_frames, long chunk, long* pb_out,
                       uint8_t* bytes_out, double* constell_out, double* cfo_out, size_t* nframes_out, void* stream)
{
    if (!c || !iq16) return fail(OFDM_ERR_INVALID, "null argument");
    const ofdm::StreamCall a{nullptr, iq16, n, max_frames, chunk, pb_out, bytes_out, constell_out, cfo_out, nframes_out,
                             stream, initial_state(c), 0, (long)n, nullptr, nullptr, 0, nullptr, nullptr};
    return ofdm::rx_stream_call(c, a);
}

int ofdm_stream_shard_margins(const ofdm_ctx* c, long* halo_out, long* tail_out)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    const long flen = c->geo.frame_len, window = 2 * c->p.t2sin_size + c->p.pr_sin_len;
    if (halo_out) *halo_out = std::max(std::max(0L, c->walk.halo_milli) * flen / 1000, flen + window + c->t2);
    if (tail_out)
        *tail_out = ofdm::WALK_SCAN_MAX + c->t2 + window + c->geo.preamble_len + c->geo.message_len + 1;
    return OFDM_OK;
}

int ofdm_walk_tuning_default(ofdm_walk_tuning* o)
{
    if (!o) return fail(OFDM_ERR_INVALID, "null argument");
    *o = ofdm_walk_tuning{};
    o->chunks_per_slot = 1;
    o->halo_milli = -1;
    o->ext_milli = 0;
    o->exact_search = 0;
    o->t2_f32 = 1;
    o->t2_margin = 4e-5;
    o->lookback = 1;
    o->pre_f32 = 1;
    return OFDM_OK;
}

int ofdm_get_walk_tuning(const ofdm_ctx* c, ofdm_walk_tuning* o)
{
    if (!c || !o) return fail(OFDM_ERR_INVALID, "null argument");
    *o = c->walk;
    return OFDM_OK;
}

int ofdm_set_walk_tuning(ofdm_ctx* c, const ofdm_walk_tuning* t)
{
    if (!c || !t) return fail(OFDM_ERR_INVALID, "null argument");
    if (t->staged_decode != 0 && t->staged_decode != 1) return fail(OFDM_ERR_INVALID, "staged_decode must be 0 or 1");
    if (t->lookback != 0 && t->lookback != 1) return fail(OFDM_ERR_INVALID, "lookback must be 0 or 1");
    if (t->pre_f32 != 0 && t->pre_f32 != 1) return fail(OFDM_ERR_INVALID, "pre_f32 must be 0 or 1");
    if (t->chunks_per_slot < 1 || t->halo_milli < -1 || t->ext_milli < 0 || !(t->t2_margin >= 0.0) ||
        t->max_rec_cap < 0)
        return fail(OFDM_ERR_INVALID, "walk tuning out of range");
    if (t->t2_margin < 4e-5 && !t->allow_uncertified)
        return fail(OFDM_ERR_INVALID, "t2_margin %g is below the certified 4e-5 (the walk could differ from the "
                                      "reference); allow_uncertified = 1 is a test-only switch", t->t2_margin);
    c->walk = *t;
    return OFDM_OK;
}

int ofdm_rx_stream_shard(ofdm_ctx* c, const double* iq, const int16_t* iq16, size_t n, const ofdm_walk_state* start,
                         long own_lo, long own_hi, size_t max_frames, long chunk, long* pb_out, uint8_t* bytes_out,
                         double* constell_out, double* cfo_out, size_t* nframes_out, long* located,
                         uint8_t* located_lag, size_t located_cap, size_t* nlocated_out, ofdm_walk_state* exit_out,
                         void* stream)
{
    if (!iq == !iq16) return fail(OFDM_ERR_INVALID, "exactly one of iq, iq16");
    if (!c || !start) return fail(OFDM_ERR_INVALID, "null argument");
    const ofdm::StreamCall a{iq, iq16, n, max_frames, chunk, pb_out, bytes_out, constell_out, cfo_out, nframes_out,
                             stream, *start, own_lo, own_hi, located, located_lag, located_cap, nlocated_out, exit_out};
    return ofdm::rx_stream_call(c, a);
}

int ofdm_set_stream_timing(ofdm_ctx* c, int on)
{
    if (!c || (on != 0 && on != 1)) return fail(OFDM_ERR_INVALID, "need a ctx and on = 0 or 1");
    HIP_TRY(hipSetDevice(c->device));
    for (ofdm::Event& ev : c->ev_phase)
        if (on && !ev) HIP_TRY(hipEventCreate(ev.put()));
    c->phase_timing = on != 0;
    c->phase_valid = false;
    return OFDM_OK;
}

int ofdm_get_stream_timing(ofdm_ctx* c, float* walk_ms, float* resolve_ms, float* decode_ms)
{
    if (!c || !walk_ms || !resolve_ms || !decode_ms) return fail(OFDM_ERR_INVALID, "null argument");
    if (!c->phase_valid)
        return fail(OFDM_ERR_INVALID, "no timed call: ofdm_set_stream_timing(ctx, 1), then a look-back stream call "
                                      "whose decode runs behind the resolve");
    HIP_TRY(hipEventSynchronize(c->ev_phase[3]));
    HIP_TRY(hipEventElapsedTime(walk_ms, c->ev_phase[0], c->ev_phase[1]));
    HIP_TRY(hipEventElapsedTime(resolve_ms, c->ev_phase[1], c->ev_phase[2]));
    HIP_TRY(hipEventElapsedTime(decode_ms, c->ev_phase[2], c->ev_phase[3]));
    return OFDM_OK;
}

int ofdm_stream_initial_state(const ofdm_ctx* c, ofdm_walk_state* out)
{
    if (!c || !out) return fail(OFDM_ERR_INVALID, "null argument");
    *out = initial_state(c);
    return OFDM_OK;
}

int ofdm_set_stream_ring(ofdm_ctx* c, long ring)
{
    if (!c) return fail(OFDM_ERR_INVALID, "null ctx");
    // R >= output_size: the smallest ring a config makes (rx_buf_size = 1,
    // Frame.cpp:221, sdr.hpp:141), the default ofdm_create sets from it
    if (ring < 0 || (ring > 0 && ring < c->geo.frame_len))
        return fail(OFDM_ERR_INVALID, "ring must be 0 or at least output_size (rx.cpp's buffer holds output_size + R, "
                                      "R = rx_buf_size * output_size)");
    c->ring = ring;
    return OFDM_OK;
}

int ofdm_shard_range(size_t total, int world, int rank, size_t* first, size_t* count)
{
    if (world < 1 || rank < 0 || rank >= world || !first || !count)
        return fail(OFDM_ERR_INVALID, "need world >= 1, 0 <= rank < world and non-null outputs");
    const size_t base = total / (size_t)world, rem = total % (size_t)world;
    *count = base + ((size_t)rank < rem ? 1 : 0);
    *first = (size_t)rank * base + std::min((size_t)rank, rem);
    return OFDM_OK;
}

int ofdm_stream_shard_plan(const ofdm_params* p, size_t n, int world, int rank, long* slice_lo, long* slice_hi,
                           long* own_lo, long* own_hi)
{
    if (!p || !slice_lo || !slice_hi || !own_lo || !own_hi) return fail(OFDM_ERR_INVALID, "null argument");
    size_t first = 0, count = 0;
    int rc = ofdm_shard_range(n, world, rank, &first, &count);
    if (rc) return rc;
    // ofdm_stream.py: stream_halo / stream_tail (the library's shard margins)
    const long L = p->fft_size + p->cp_size, t2 = p->t2sin_size, pre = L * p->num_pr_symb, msg = L * p->num_symb;
    const long flen = t2 + pre + msg, window = 2 * t2 + p->pr_sin_len;
    const long halo = std::max(3 * flen, flen + window + t2);
    const long tail = ofdm::WALK_SCAN_MAX + t2 + window + pre + msg + 1;
    *own_lo = (long)first;
    *own_hi = (long)(first + count);
    *slice_lo = std::max(0L, *own_lo - halo);
    *slice_hi = std::min((long)n, *own_hi + tail);
    return OFDM_OK;
}

int ofdm_reduce_counters(ofdm_ctx* c, int64_t* counters, size_t count, void* comm, void* stream)
{
    if (!c || !counters || !comm) return fail(OFDM_ERR_INVALID, "null argument");
    // RCCL is loaded on first use (the core library does not link it): the
    // one collective of a multi-GPU job, ncclAllReduce(int64, sum)
    using AllReduce = int (*)(const void*, void*, size_t, int, int, void*, hipStream_t);
    using ErrStr = const char* (*)(int);
    static std::mutex mu;
    static AllReduce all_reduce = nullptr;
    static ErrStr err_str = nullptr;
    {
        std::lock_guard<std::mutex> g(mu);
        if (!all_reduce) {
            void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
            if (!h) return fail(OFDM_ERR_UNSUPPORTED, "RCCL (librccl.so) not found: %s", dlerror());
            all_reduce = reinterpret_cast<AllReduce>(dlsym(h, "ncclAllReduce"));
            err_str = reinterpret_cast<ErrStr>(dlsym(h, "ncclGetErrorString"));
            if (!all_reduce) return fail(OFDM_ERR_UNSUPPORTED, "librccl.so has no ncclAllReduce");
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    const int r = all_reduce(counters, counters, count, kRcclInt64, kRcclSum, comm, (hipStream_t)stream);
    if (r != 0) return fail(OFDM_ERR_HIP, "ncclAllReduce: %s", err_str ? err_str(r) : "error");
    return OFDM_OK;
}

int ofdm_stream_report_pack(int rank, long slice_lo, long own_lo, long own_hi, const long* located,
                            const uint8_t* located_lag, size_t nlocated, const ofdm_walk_state* exit_state,
                            int true_start, size_t cap, int64_t* row)
{
    // ofdm_stream.py pack_report: header, then the walk's first and last cap
    // located frames, each as 2*pb + lag (-1: empty)
    if (!row || !exit_state || (nlocated && !located) || cap < 1) return fail(OFDM_ERR_INVALID, "null argument or cap 0");
    const size_t H = OFDM_STREAM_REPORT_HEADER;
    const int64_t head[H] = {rank, slice_lo, own_lo, own_hi, exit_state->pos, exit_state->ring_end, true_start ? 1 : 0};
    std::copy(head, head + H, row);
    std::fill(row + H, row + H + 2 * cap, (int64_t)-1);
    auto key = [&](size_t i) { return 2 * (int64_t)located[i] + (located_lag && located_lag[i] ? 1 : 0); };
    const size_t nh = std::min(nlocated, cap);
    for (size_t i = 0; i < nh; ++i) row[H + i] = key(i);
    if (nlocated > cap)
        for (size_t i = 0; i < cap; ++i) row[H + cap + i] = key(nlocated - cap + i);
    return OFDM_OK;
}

int ofdm_stream_stitch_plan(const int64_t* rows, int world, size_t cap, long t2, int* rank_out,
                            ofdm_walk_state* start_out)
{
    // ofdm_stream.py unpack_report + stitch_plan + rewalk_start
    if (!rows || !rank_out || !start_out || world < 1 || cap < 1 || t2 < 1)
        return fail(OFDM_ERR_INVALID, "need rows, outputs, world >= 1, cap >= 1, t2sin_size >= 1");
    const size_t H = OFDM_STREAM_REPORT_HEADER, len = H + 2 * cap;
    auto keys = [&](int r) {  // the rank's located keys (2*pb + lag), sorted, unique
        std::vector<int64_t> k;
        for (size_t i = H; i < len; ++i)
            if (rows[r * len + i] >= 0) k.push_back(rows[r * len + i]);
        std::sort(k.begin(), k.end());
        k.erase(std::unique(k.begin(), k.end()), k.end());
        return k;
    };
    *rank_out = -1;
    *start_out = ofdm_walk_state{-1, 0};
    for (int r = 1; r < world; ++r) {
        const int64_t* cur = rows + r * len;
        const int64_t* prev = rows + (r - 1) * len;
        if (cur[6]) continue;  // walked from a true state
        const std::vector<int64_t> kc = keys(r), kp = keys(r - 1);
        int64_t first = INT64_MAX;  // the first owned frame's preamble start
        for (int64_t k : kc)
            if ((k >> 1) >= cur[2] && (k >> 1) < cur[3]) first = std::min(first, k >> 1);
        std::vector<int64_t> common;
        std::set_intersection(kc.begin(), kc.end(), kp.begin(), kp.end(), std::back_inserter(common));
        bool ok = false;
        for (int64_t k : common) ok = ok || (k >> 1) <= first;
        if (ok) continue;
        *rank_out = r;
        if (prev[4] < 0) return OFDM_OK;  // the true walk ran out of samples before this core
        long pos = (long)prev[4];
        const long slice_lo = (long)cur[1];
        if (pos < slice_lo) pos += (slice_lo - pos + t2 - 1) / t2 * t2;  // forward on its own T2 grid
        *start_out = ofdm_walk_state{pos, (long)prev[5]};
        return OFDM_OK;
    }
    return OFDM_OK;
}

int ofdm_device_count(int* count)
{
    if (!count) return fail(OFDM_ERR_INVALID, "null argument");
    *count = 0;
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    *count = n;
    return OFDM_OK;
}

int ofdm_get_stream_ring(const ofdm_ctx* c, long* ring)
{
    if (!c || !ring) return fail(OFDM_ERR_INVALID, "null argument");
    *ring = c->ring;
    return OFDM_OK;
}

}  // extern "C"
