// ofdm_ctx.hpp — the modem context behind the C-ABI's opaque ofdm_ctx, and the
// helpers that the three host files share: ofdm_create.cpp (the context's life
// cycle and its tables), ofdm_capi.cpp (the entry points) and
// ofdm_stream_call.cpp (the stream receiver). Every HIP resource of the context
// is held by an owner (ofdm_owned.hpp), so deleting the context releases them
// all. Host code only: no .hip file includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include <complex>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/ofdm_mi355x.h"
#include "ofdm_internal.hpp"
#include "ofdm_owned.hpp"

using cd = std::complex<double>;

struct ofdm_ctx {
    template <class T>
    using DevBuf = ofdm::DevBuf<T>;
    ofdm_params p{};
    int device = 0;
    int logn = 0;
    int N = 0, D = 0, P = 0, cp = 0, S = 0, k = 0, L = 0, seg = 0, npr = 0, t2 = 0;
    ofdm_geometry geo{};
    // host constants
    std::vector<cd> t2_symbol, ofdm_preamble, mod_preamble, templ;
    std::vector<uint8_t> preamble_bytes;
    std::vector<double> t2_mask;
    // device tables
    DevBuf<double2> d_tw;
    DevBuf<int> d_data_bin;
    DevBuf<int> d_data_slot;
    DevBuf<int> d_pilot_bin;
    DevBuf<int> d_bin_map;
    DevBuf<int> d_rx_pack;
    DevBuf<int> d_pilot_swz;
    DevBuf<int> d_tx_code;
    // tx dead-group masks (ofdm_internal.hpp tx_dead_masks); d_tx_dead stays
    // null when no wave has a dead group. tx_sparse: ofdm_tx_sparse's switch
    std::vector<int> tx_code;
    std::vector<unsigned> tx_dead;
    DevBuf<unsigned> d_tx_dead;
#ifndef OFDM_TX_SPARSE_DEFAULT  // 0: an A/B build (tools/build_variant.sh) that maps every group
#define OFDM_TX_SPARSE_DEFAULT 1
#endif
    bool tx_sparse = OFDM_TX_SPARSE_DEFAULT != 0;
    DevBuf<double2> d_const;
    DevBuf<double2> d_const_bpsk;
    // decide_select's thresholds (the rx emit's fast path, k = 2), found on
    // the device at creation; dec_fast = false: the scan's checks failed or
    // k is not 2, and rx keeps the decision arithmetic
    double dec_tau[3] = {};
    bool dec_fast = false;
    DevBuf<double2> d_header;      // T2 + preamble
    DevBuf<double2> d_preamble;    // ofdm_preamble (preamble_len)
    DevBuf<double2> d_templ;       // pr_sin_len
    DevBuf<double2> d_tspec;       // WALK_FFT_M template spectrum (stream walker FFT search)
    DevBuf<float2> d_tspec32;      // the same rounded to FP32 (the search's FP32 tier)
    DevBuf<double2> d_twm;         // WALK_FFT_M twiddles
    double tspec_max = 0.0;
    DevBuf<double2> d_modpre;      // D*npr
    DevBuf<double> d_t2mask;       // t2 size
    DevBuf<double2> d_t2tw;        // t2-size twiddles (T2 detector)
    DevBuf<int> d_first;           // T2 detector min-block scratch
    int t2_logn = -1;              // T2sin_size = 2^t2_logn, else -1 (detector unsupported)
    struct CfoPlan {               // pilot_freq_sinh on a form of nsym symbols
        int nsym = 0, logm = -1, g = 0;
        DevBuf<double2> tw_sub;
        DevBuf<double2> tw_full;
        DevBuf<int> borders;
    };
    std::vector<CfoPlan> cfo_plans;
    // scratch that only grows (ofdm::grow / ofdm::grow_host): an owner and its size
    template <class Own>
    struct Grown {
        Own p;
        size_t bytes = 0;
    };
    using Grow = Grown<DevBuf<void>>;
    using GrowHost = Grown<ofdm::HostBlock>;
    // ofdm_sync_frames' CFO estimates where the caller takes none, and the
    // staged-rx scratch (only for num_symb > 8 or D > N/2)
    Grow d_cfo_scratch, d_scratch;
    // ofdm_rx_stream scratch (grown on demand): walker records, frame batch,
    // channel estimates, frame starts
    Grow s_walk, s_batch, s_chan, s_pbs;
    // find_preamble's split form: magnitudes and per-start counters (zero
    // between launches) for up to PRE_SCRATCH_STARTS start indices per call
    static constexpr size_t PRE_SCRATCH_STARTS = 64;
    DevBuf<double> d_pre_hv;
    DevBuf<unsigned> d_pre_done;
    // pinned host staging for the walk records and the frame list (pageable
    // copies go through a driver bounce buffer and synchronise twice)
    GrowHost h_walk, h_frames;
    hipStream_t h_frames_stream = nullptr;  // stream of the last copy out of h_frames
    bool h_frames_used = false;
    DevBuf<int> d_queue;           // walker chunk counter (zero between calls)
    // rx dynamic-frame counters {next, done}, zero between launches: one slot
    // per HIP stream that launched rx on this context (launches on one stream
    // run in order, so each slot is reset by the launch before the next uses
    // it); streams past RX_QUEUE_SLOTS run with a static frame order
    static constexpr int RX_QUEUE_SLOTS = 32;
    DevBuf<int> d_rxq;             // RX_QUEUE_SLOTS x 16 ints (one 64-B line each)
    hipStream_t rxq_stream[RX_QUEUE_SLOTS] = {};
    bool rxq_live[RX_QUEUE_SLOTS] = {};  // slot bound to rxq_stream[i] (false: freed by ofdm_stream_destroy)
    int rxq_used = 0;
    ofdm_walk_tuning walk{};       // stream walker settings (ofdm_set_walk_tuning)
    long ring = 0;                 // rx.cpp's SDR ring R (ofdm_set_stream_ring; 0: the continuous walk)
    bool queue_zero = false;       // the last stream call's compaction left the walker counter zero
    ofdm::Event ev_call;           // recorded on call_stream when a stream call comes on another stream
    hipStream_t call_stream = nullptr;  // the last stream call's HIP stream
    bool call_valid = false;       //   (call_stream set)
    ofdm::Event ev_walk;           // walk records landed in h_walk
    ofdm::Event ev_wdone;          // the walk kernel finished (caller's stream)
    ofdm::Stream side;             // copies the walk records out beside the decode
    // look-back walk: per-chunk publication counts (zero between calls: the
    // resolve kernel clears them), the true walk's records for shard reports,
    // and the resolve kernel's status block (page-locked, written by the kernel)
    Grow s_pub, s_chain;
    GrowHost h_status;
    bool pub_zero = false;         // every s_pub word is zero
    // per-phase device times of the last look-back stream call
    // (ofdm_set_stream_timing): events before the walk, after the walk, after
    // the resolve and after the decode, on the call's stream
    bool phase_timing = false;
    bool phase_valid = false;
    ofdm::Event ev_phase[4];

    ofdm::DevTables tables(bool bpsk) const
    {
        ofdm::DevTables t;
        t.tw = d_tw;
        t.data_bin = d_data_bin;
        t.data_slot = d_data_slot;
        t.pilot_bin = d_pilot_bin;
        t.bin_map = d_bin_map;
        t.rx_pack = d_rx_pack;
        t.pilot_swz = d_pilot_swz;
        t.tx_code = d_tx_code;
        t.constell = bpsk ? d_const_bpsk : d_const;
        return t;
    }
};

namespace ofdm {

// ---- defined in ofdm_create.cpp ----
// pilot_freq_sinh plan for a form of nsym symbols (built on first use)
int cfo_plan(ofdm_ctx* c, int nsym, ofdm_ctx::CfoPlan** out, hipStream_t st);

// ---- defined in ofdm_capi.cpp ----
// sets ofdm_last_error's text for this thread; returns `code`
int fail(int code, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return ::ofdm::hip_fail(_e, #expr); \
    } while (0)

bool aligned16(const void* p);
// device scratch / pinned host staging that only grows (contents not preserved)
int grow(ofdm_ctx* c, ofdm_ctx::Grow& g, size_t need);
int grow_host(ofdm_ctx* c, ofdm_ctx::GrowHost& g, size_t need);
// whether `st` is being captured into a hipGraph, and the refusal of a call
// that a capture does not allow
bool capturing(hipStream_t st);
int capture_refused(const char* what);
// rx.cpp's initial walk state
ofdm_walk_state initial_state(const ofdm_ctx* c);

// ---- defined in ofdm_stream_call.cpp ----
// One call of ofdm_rx_stream / ofdm_rx_stream_i16 / ofdm_rx_stream_shard:
// exactly one of iq, iq16 is set. The walk starts at state `start`; frames
// located with pb in [own_lo, own_hi) are decoded (the whole stream: start =
// the initial state, own_lo = 0, own_hi = n). Outputs as in ofdm_mi355x.h.
struct StreamCall {
    const double* iq;
    const int16_t* iq16;
    size_t n, max_frames;
    long chunk;  // <= 0: one chunk per resident walker slot
    long* pb_out;
    uint8_t* bytes_out;
    double* constell_out;
    double* cfo_out;
    size_t* nframes_out;
    void* stream;
    ofdm_walk_state start;
    long own_lo, own_hi;
    long* located;
    uint8_t* located_lag;
    size_t located_cap;
    size_t* nlocated_out;
    ofdm_walk_state* exit_out;
};
int rx_stream_call(ofdm_ctx* c, const StreamCall& a);

}  // namespace ofdm
