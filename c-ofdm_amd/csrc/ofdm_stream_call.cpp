// ofdm_stream_call.cpp — the host side of one stream-receiver call
// (ofdm_rx_stream / ofdm_rx_stream_i16 / ofdm_rx_stream_shard, whose wrappers
// in ofdm_capi.cpp fill a StreamCall): validation, the chunk plan, the walk
// launch, and the two ways to finish it: the look-back walk resolved on the
// device (finish_lookback), or the halo walk stitched on the host
// (finish_halo, with the list logic of ofdm_stream_stitch.hpp). Every kernel
// is in ofdm_sync.hip / ofdm_kernels.hip / ofdm_stream_wide.hip.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ofdm_ctx.hpp"
#include "ofdm_stream_stitch.hpp"
#include "ofdm_sync.hpp"

namespace ofdm {
namespace {

static_assert(REC_LAG_BIT == WALK_REC_LAG && REC_PB_MASK == WALK_REC_PB, "ofdm_stream_stitch.hpp's record bits");

// one decode launch takes at most this much internal scratch (channel
// estimates and ramps, or gathered frames); longer lists go in batches, and
// only a list that fits one batch is decoded speculatively
constexpr size_t DECODE_BATCH_BYTES = (size_t)256 << 20;

// OFDM_STREAM_DEBUG: one stderr line per call on how it went (asked once per call)
bool stream_debug() { return getenv("OFDM_STREAM_DEBUG") != nullptr; }

// OFDM_DECODE_BATCH_FRAMES=<n>, n >= 1 (test only, asked once per call): at
// most n frames per decode launch, so that a short stream takes the batched,
// non-speculative decode of a capture whose scratch passes DECODE_BATCH_BYTES.
// A value that is not an integer >= 1 is ignored. Returns 0 for "no cap"
size_t decode_batch_cap()
{
    const char* s = getenv("OFDM_DECODE_BATCH_FRAMES");
    if (!s || !*s) return 0;
    char* end = nullptr;
    const long long v = strtoll(s, &end, 10);
    return (*end == 0 && v >= 1) ? (size_t)v : 0;
}

// Frames per decode launch for `per` bytes of scratch per frame: what fits
// DECODE_BATCH_BYTES (at least one), capped by the test hook
size_t batch_frames(size_t per, size_t cap)
{
    const size_t n = std::max<size_t>(1, DECODE_BATCH_BYTES / per);
    return cap ? std::min(n, cap) : n;
}

long preamble_len(const ofdm_ctx* c) { return (long)c->L * c->npr; }
long message_len(const ofdm_ctx* c) { return (long)c->L * c->S; }

// Validation only; a valid call's outputs read "no frames, no exit state"
// until a later stage writes them.
int check_stream_call(const ofdm_ctx* c, const StreamCall& a)
{
    if (!c || (!a.iq && !a.iq16) || !a.nframes_out) return fail(OFDM_ERR_INVALID, "null argument");
    *a.nframes_out = 0;
    if (a.nlocated_out) *a.nlocated_out = 0;
    if (a.exit_out) *a.exit_out = ofdm_walk_state{-1, 0};
    const long R = c->ring, flen0 = c->geo.frame_len;
    const long start = a.start.pos;
    // ring mode: the walk may start in rx.cpp's zero header before the first
    // SDR buffer ([-output_size, 0)); its ring end lies ahead of it, within R.
    // An exit state may also lie a little past its ring end: a walk that
    // crossed own_hi inside a T2 scan whose next block leaves the ring (the
    // state's next step is the refill, pos = ring_end, rx.cpp:137-145)
    const long past = WALK_SCAN_MAX + c->t2;
    if (R > 0 ? (start < -flen0 || a.start.ring_end <= start - past || a.start.ring_end > start + R + flen0)
              : start < 0)
        return fail(OFDM_ERR_INVALID, "start state out of range (ring mode: -output_size <= pos, pos - %ld < ring_end "
                                      "<= pos + R + output_size)", past);
    if (a.own_lo < 0 || a.own_lo > a.own_hi || a.own_hi > (long)a.n)
        return fail(OFDM_ERR_INVALID, "need 0 <= own_lo <= own_hi <= n");
    if (c->t2_logn < 6 || c->t2_logn > 11) return fail(OFDM_ERR_UNSUPPORTED, "stream walk needs T2sin_size = 2^a, 64..2048");
    // the walker's LDS, as plan_walk and launch_stream_walk will ask for it
    const size_t lds = stream_walk_lds(c->t2_logn, (int)c->p.pr_sin_len, (int)(2 * c->p.t2sin_size + c->p.pr_sin_len),
                                       c->d_tspec != nullptr);
    if (lds > STREAM_WALK_MAX_LDS)
        return fail(OFDM_ERR_UNSUPPORTED, "stream walk: T2sin_size = %ld with pr_sin_len = %ld needs %zu bytes of LDS "
                                          "(limit %zu)", (long)c->p.t2sin_size, (long)c->p.pr_sin_len, lds,
                    STREAM_WALK_MAX_LDS);
    if ((a.iq && !aligned16(a.iq)) || (a.iq16 && ((uintptr_t)a.iq16 & 3)) ||
        (a.constell_out && !aligned16(a.constell_out)))
        return fail(OFDM_ERR_INVALID, "misaligned buffer (complex<double> 16 B, complex<int16> 4 B)");
    if (a.n > (size_t)1 << 40) return fail(OFDM_ERR_INVALID, "stream too long");
    return OFDM_OK;
}

// How the walk of [own_lo, own_hi) is cut into chunks.
// Per-context tuning (ofdm_set_walk_tuning): chunks per walker slot, walk-in
// halo and walk-on extension in 1/1000 frames, look-back stitching. Look-back
// (the default): chunks start at their core (no walk-in) and each walks on
// past its core end until its walk joins the next chunk's (a device-side
// check of the records that chunk publishes); the chain of joined walks is
// the sequential walk, resolved on the device. Without it (lookback = 0, or
// force_halo: the fallback when a walker's records overflow): each chunk
// walks in from a 3-frame halo and the host stitches the walks, re-walking a
// chunk whose walk-in did not meet the true walk.
struct WalkPlan {
    long slots;       // walkers resident at once
    long chunk;       // core samples per chunk
    long nchunks;
    bool force_halo;  // no look-back, whatever the tuning says
    bool lbk;         // the look-back walk
    long halo, ext;   // walk-in before the core, walk-on past it (samples)
    int max_rec;      // records per chunk
};

// `chunk` <= 0: one chunk per resident walker slot, each >= 8 frames. Pure
// arithmetic on the call and the context (its one query: stream_walk_slots).
int plan_walk(const ofdm_ctx* c, const StreamCall& a, long chunk, bool force_halo, WalkPlan* out)
{
    WalkPlan p{};
    const long flen = c->geo.frame_len, msg = message_len(c), start = a.start.pos;
    p.slots = stream_walk_slots(c->t2_logn, (int)c->p.pr_sin_len, (int)(2 * c->p.t2sin_size + c->p.pr_sin_len),
                                c->d_tspec != nullptr);
    const ofdm_walk_tuning& tu = c->walk;
    const long qper = std::max(1L, tu.chunks_per_slot);
    const long span_w = a.own_hi - a.own_lo;  // the chunk cores tile [own_lo, own_hi)
    if (chunk <= 0) chunk = std::max(8 * flen, (span_w + p.slots * qper - 1) / (p.slots * qper));
    p.chunk = std::max(chunk, (long)c->t2);
    p.nchunks = std::max(1L, (span_w + p.chunk - 1) / p.chunk);
    if (p.nchunks > 1 << 20) return fail(OFDM_ERR_INVALID, "chunk too small for this stream");
    // look-back needs a resolvable chunk count and per-chunk record counts
    // below 2^14 (the resolve kernel's packing): else the halo walk
    p.force_halo = force_halo;
    p.lbk = tu.lookback && !force_halo && p.nchunks <= RESOLVE_MAX_CHUNKS &&
            (2 * p.chunk + std::max(0L, a.own_lo - start)) / msg < 8192;
    p.halo = (tu.halo_milli < 0 ? (p.lbk ? 0L : 3000L) : tu.halo_milli) * flen / 1000;
    p.ext = std::max(0L, tu.ext_milli) * flen / 1000;
    // each located frame advances the walk by > message_len, and a walker can
    // walk on past its core end by ext plus one scan step (WALK_SCAN_MAX
    // samples) and the preamble window: this many records always suffice
    // (chunk 0 walks in from `start`, the others a halo before their core).
    // A look-back walker may walk on through the next core too (its walk met
    // no record of that chunk's); one more overflows: the host falls back
    p.max_rec = (int)(((p.lbk ? 2 : 1) * p.chunk + std::max(p.halo, a.own_lo - start) + std::max(p.ext, 2 * flen) +
                       WALK_SCAN_MAX + 2 * c->p.t2sin_size + c->p.pr_sin_len) / msg + (p.lbk ? 8 : 4));
    // test hook: a smaller record buffer makes look-back walkers overflow
    // (the halo walk, which the cap does not touch, then takes the call)
    if (p.lbk && tu.max_rec_cap > 0) p.max_rec = std::min(p.max_rec, tu.max_rec_cap);
    *out = p;
    return OFDM_OK;
}

// The walk scratch, one layout for the device buffer (s_walk) and its host
// mirror (h_walk):
//   records | exit positions | exit ring ends | re-walk start (pos, ring end) | counts | re-walk id
//   (in 64 B of slack) | in-core counts | first indices | look-back links
// The mirror holds the first walk_b bytes (no links).
struct WalkView {
    long* rec;        // [chunk][max_rec]
    long* exit_pos;   // [chunk]
    long* exit_ring;  // [chunk]
    long* start;      // one re-walk start state (pos, ring end)
    int* nrec;        // [chunk]
    int* ids;         // one re-walk chunk id
    int* ncore;       // [chunk]
    int* first_in;    // [chunk]
    int* link;        // [chunk][3] (device only)
};

struct WalkBuffers {
    long nchunks = 0;
    size_t rec_b = 0, walk_b0 = 0, walk_b = 0, link_b = 0;

    WalkBuffers(long nchunks_, int max_rec) : nchunks(nchunks_)
    {
        rec_b = (size_t)nchunks * max_rec * sizeof(long);
        walk_b0 = rec_b + (size_t)nchunks * (2 * sizeof(long) + sizeof(int)) + 2 * sizeof(long) + 64;
        walk_b = walk_b0 + 2 * (size_t)nchunks * sizeof(int);  // + in-core counts and first indices
        link_b = 3 * (size_t)nchunks * sizeof(int);            // + look-back links
    }
    size_t device_bytes() const { return walk_b + link_b; }
    size_t host_bytes() const { return walk_b; }
    WalkView view(void* base) const
    {
        char* b = static_cast<char*>(base);
        WalkView v{};
        v.rec = reinterpret_cast<long*>(b);
        v.exit_pos = reinterpret_cast<long*>(b + rec_b);
        v.exit_ring = v.exit_pos + nchunks;
        v.start = v.exit_ring + nchunks;
        v.nrec = reinterpret_cast<int*>(v.start + 2);
        v.ids = v.nrec + nchunks;
        v.ncore = reinterpret_cast<int*>(b + walk_b0);
        v.first_in = v.ncore + nchunks;
        v.link = reinterpret_cast<int*>(b + walk_b);
        return v;
    }
};

// One attempt's walk: its plan, its scratch and the launch arguments
struct Walk {
    WalkPlan plan;
    WalkBuffers buf;
    WalkView dev;
    WalkArgs args{};
    bool timed = false;  // phase events around the kernels (measurement calls only)

    explicit Walk(const WalkPlan& p) : plan(p), buf(p.nchunks, p.max_rec), dev{} {}
};

int fill_walk_args(ofdm_ctx* c, const StreamCall& a, const WalkPlan& p, const WalkView& d, WalkArgs& w)
{
    const ofdm_walk_tuning& tu = c->walk;
    const long R = c->ring, flen = c->geo.frame_len;
    w.exact_only = tu.exact_search != 0;
    w.tw_m = c->d_twm;
    w.tspec = c->d_tspec;  // nullptr: direct certified search
    w.tspec_max = c->tspec_max;
    w.tspec32 = tu.pre_f32 ? c->d_tspec32 : nullptr;  // FP32 tier of the FFT search
    w.iq = reinterpret_cast<const double2*>(a.iq);
    w.iq16 = reinterpret_cast<const short2*>(a.iq16);
    w.n = (long)a.n;
    w.t2tw = c->d_t2tw;
    const int sm = (int)c->p.smooth, f1 = (int)c->p.t2_sin_f1, f2 = (int)c->p.t2_sin_f2;
    w.a1 = std::max(0, f1 - sm);
    w.b1 = std::min(c->t2 - 1, f1 + sm);
    w.a2 = std::max(0, f2 - sm);
    w.b2 = std::min(c->t2 - 1, f2 + sm);
    w.t2_level = (double)c->p.t2_sin_level / 1000;
    // FP32 T2 screen (certified, FP64 re-evaluation of uncertain steps)
    w.t2_f32 = tu.t2_f32 != 0;
    w.t2_margin = tu.t2_margin;
    w.templ = c->d_templ;
    w.L = (int)c->p.pr_sin_len;
    w.cycles = (int)(2 * c->p.t2sin_size + c->p.pr_sin_len);
    w.pr_level = (double)c->p.pr_level / 1000;
    w.pre = preamble_len(c);
    w.msg = message_len(c);
    w.chunk = p.chunk;
    w.halo = p.halo;
    w.start = a.start.pos;
    w.ring = R;
    w.out_len = flen;
    w.start_ring_end = a.start.ring_end;
    w.ring_phase = R > 0 ? ((a.start.ring_end % R) + R) % R : 0;
    w.exit_ring = d.exit_ring;
    w.core_lo = a.own_lo;
    w.core_hi = a.own_hi;
    w.ext = p.ext;
    // A chunk whose core end falls inside a T2 scan (its last frame well
    // before the end, e.g. a frame the reference's walk misses) walks on to
    // the next frame it locates: the next chunk's walk locates that frame
    // too, so the two sync without a serial re-walk (2048 chunks of config 4:
    // one re-walk per call without this).
    w.ext_scan = std::max(p.ext, 2 * flen);
    w.max_rec = p.max_rec;
    w.rec = d.rec;
    w.nrec = d.nrec;
    w.exit_pos = d.exit_pos;
    w.ncore = d.ncore;
    w.first_in = d.first_in;
    // the walkers take chunks from a queue: one resident round of workgroups
    // drains it, slower walkers taking fewer chunks. The counter is zeroed by
    // the previous call's compaction (stream order), else by launch_walk.
    if (!c->d_queue) {
        HIP_TRY(hipMalloc((void**)c->d_queue.put(), 64));
        c->queue_zero = false;
    }
    w.queue = c->d_queue;
    w.nchunks = p.nchunks;
    return OFDM_OK;
}

// The previous stream call's work must be done before this one rewrites
// the ctx's scratch (walk records, compacted list, channel): its decodes
// read them. On the same stream that is stream order; on another stream
// this call waits for an event recorded now on the previous call's stream
// (behind that call's decodes; header: overlapping stream calls take two
// contexts). Recorded here rather than at the end of every call: an event
// between two dependent kernels of one stream costs a launch gap (the
// next call's walker started ~15-25 us after the decode ended).
int order_after_previous_call(ofdm_ctx* c, hipStream_t st)
{
    if (c->call_valid && c->call_stream != st) {
        if (!c->ev_call) HIP_TRY(hipEventCreateWithFlags(c->ev_call.put(), hipEventDisableTiming));
        if (hipEventRecord(c->ev_call, c->call_stream) == hipSuccess) {
            HIP_TRY(hipStreamWaitEvent(st, c->ev_call, 0));
        } else {
            (void)hipGetLastError();  // that stream is gone (destroyed): wait for the device instead
            HIP_TRY(hipDeviceSynchronize());
        }
    }
    c->call_stream = st;
    c->call_valid = true;
    return OFDM_OK;
}

// diagnostics: OFDM_WALK_PROF=<file> appends one JSON line per walk launch
// (a look-back walk that overflows and its halo walk: two; a re-walk: none)
// with every chunk's walker timeline (WalkArgs::prof). T2sin_size = 256 only
// (stream_walk_has_prof): other sizes have no diagnostics walker, no line
int dump_walk_prof(const char* path, const long* d_prof, const WalkPlan& p, hipStream_t st)
{
    std::vector<long> hp((size_t)p.nchunks * WALK_PROF_FIELDS);
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(hp.data(), d_prof, hp.size() * sizeof(long), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(path, "a")) {
        fprintf(f, "{\"nchunks\": %ld, \"chunk\": %ld, \"lookback\": %d, \"grid\": %ld, \"fields\": "
                   "[\"t0\", \"t_core\", \"t_end\", \"ext_frames\", \"waits\", \"block\", \"xcc\", \"nrec\", "
                   "\"t2_ticks\", \"pre_ticks\", \"scan_steps\", \"fp64_evals\", \"searches\", \"hw_id\"], "
                   "\"chunks\": [", p.nchunks, p.chunk, (int)p.lbk, std::min(p.nchunks, p.slots));
        for (long k = 0; k < p.nchunks; ++k) {
            fprintf(f, "%s[", k ? "," : "");
            for (int i = 0; i < WALK_PROF_FIELDS; ++i)
                fprintf(f, "%s%ld", i ? "," : "", hp[(size_t)k * WALK_PROF_FIELDS + i]);
            fprintf(f, "]");
        }
        fprintf(f, "]}\n");
        fclose(f);
    }
    return OFDM_OK;
}

// the walk kernel, between the first two phase events of a timed call
int launch_walk_kernel(ofdm_ctx* c, const Walk& wk, hipStream_t st)
{
    if (wk.timed) HIP_TRY(hipEventRecord(c->ev_phase[0], st));
    hipError_t e = launch_stream_walk(c->t2_logn, wk.args, std::min(wk.plan.nchunks, wk.plan.slots), st);
    if (e != hipSuccess) return hip_fail(e, "stream_walk launch");
    if (wk.timed) HIP_TRY(hipEventRecord(c->ev_phase[1], st));
    return OFDM_OK;
}

// Zero what the walkers count in (unless the previous call left it zero),
// then the walk.
int launch_walk(ofdm_ctx* c, Walk& wk, hipStream_t st)
{
    WalkArgs& w = wk.args;
    const long nchunks = wk.plan.nchunks;
    int rc;
    if (!c->queue_zero) HIP_TRY(hipMemsetAsync(w.queue, 0, sizeof(int), st));
    c->queue_zero = false;
    if (wk.plan.lbk) {
        if (c->s_pub.bytes < (size_t)nchunks * sizeof(int)) {
            if ((rc = grow(c, c->s_pub, (size_t)std::max(nchunks, 2048L) * sizeof(int)))) return rc;
            c->pub_zero = false;
        }
        if (!c->pub_zero) HIP_TRY(hipMemsetAsync(c->s_pub.p, 0, c->s_pub.bytes, st));
        c->pub_zero = false;  // until the resolve kernel clears it again
        w.lookback = 1;
        w.pub = static_cast<int*>(c->s_pub.p.get());
        w.link = wk.dev.link;
    }
    // only the T2 size with a diagnostics walker writes a timeline; any other
    // runs the normal walk and adds no line
    const char* prof_path = stream_walk_has_prof(c->t2_logn) ? getenv("OFDM_WALK_PROF") : nullptr;
    long* d_prof = nullptr;
    if (prof_path) HIP_TRY(hipMalloc((void**)&d_prof, (size_t)nchunks * WALK_PROF_FIELDS * sizeof(long)));
    w.prof = d_prof;
    c->phase_valid = false;
    wk.timed = c->phase_timing && wk.plan.lbk;  // events between the kernels: measurement calls only
    rc = launch_walk_kernel(c, wk, st);
    if (d_prof) {
        if (!rc) rc = dump_walk_prof(prof_path, d_prof, wk.plan, st);
        const hipError_t e = hipFree(d_prof);  // whatever failed above
        if (!rc && e != hipSuccess) rc = hip_fail(e, "hipFree(d_prof)");
        w.prof = nullptr;  // a re-walk copies these arguments
    }
    return rc;
}

// The decode back end of one call
struct Decode {
    ofdm_ctx* c;
    const StreamCall* a;
    hipStream_t st;
    ofdm_ctx::CfoPlan* pl;  // pilot_freq_sinh plan of the preamble form (fused)
    bool fused;             // the fused kernels take this geometry
    size_t per;             // their scratch per frame: channel, ramps, CFO
    size_t batch_cap;       // OFDM_DECODE_BATCH_FRAMES (0: none)
    long npts;              // constellation points per frame
};

// Fused decode: three kernels read each frame from the stream in place
// (pilot_freq_sinh; the other sync stages' parameters + chan_char_lq;
// rx with the corrections applied on load), no frame copy, no corrected
// copy. Needs the register-window rx and a pilot_freq_sinh plan.
bool fused_geometry(ofdm_ctx* c, hipStream_t st, ofdm_ctx::CfoPlan** pl)
{
    return c->S <= RX_SMAX && c->D <= RX_DPT * (c->N / 8) && c->P <= c->N / 8 && c->npr == 1 && c->S + 1 <= 64 &&
           c->L % (c->N / 8) == 0 && c->L / (c->N / 8) <= 16 &&
           c->cp <= 2 * (c->N / 8) &&  // stream_params_kernel: CP template in 2 registers
           cfo_plan(c, c->npr, pl, st) == OFDM_OK;
}

Decode decode_backend(ofdm_ctx* c, const StreamCall& a, hipStream_t st, size_t batch_cap)
{
    Decode d{c, &a, st, nullptr, false, 0, batch_cap, 0};
    d.fused = fused_geometry(c, st, &d.pl);
    d.per = (size_t)c->D * sizeof(double2) + (size_t)c->S * CORR_PER_SYM * sizeof(double2) + sizeof(double);
    d.npts = (long)c->D * c->S;
    return d;
}

// Whether up to `ub` frames may be decoded behind the walk before the host
// knows the list: the fused kernels (they bound the list by a device count),
// in one batch
bool speculative_ok(const Decode& d, size_t ub) { return d.fused && ub > 0 && ub <= batch_frames(d.per, d.batch_cap); }

// frames [0, nb_total) of d_list (device count d_cnt, if set, bounds them further)
int decode_fused(const Decode& d, const long* d_list, size_t nb_total, const long* d_cnt)
{
    ofdm_ctx* c = d.c;
    const StreamCall& a = *d.a;
    const ofdm_ctx::CfoPlan* pl = d.pl;
    const size_t bmax = batch_frames(d.per, d.batch_cap);
    const size_t nb0 = std::min(nb_total, bmax);
    int r2;
    if ((r2 = grow(c, c->s_chan, nb0 * d.per))) return r2;
    double2* chan = static_cast<double2*>(c->s_chan.p.get());
    double2* corr = chan + nb0 * c->D;
    double* cfo_tmp = reinterpret_cast<double*>(corr + nb0 * c->S * CORR_PER_SYM);
    for (size_t f0 = 0; f0 < nb_total; f0 += nb0) {
        const size_t nb = std::min(nb0, nb_total - f0);
        double* cfo = a.cfo_out ? a.cfo_out + f0 : cfo_tmp;
        CfoArgs ca{};
        ca.x = reinterpret_cast<const double2*>(a.iq);
        ca.x16 = reinterpret_cast<const short2*>(a.iq16);
        ca.starts = d_list + f0;
        ca.nframes = (long)nb;
        ca.tw_sub = pl->tw_sub;
        ca.tw_full = pl->tw_full;
        ca.borders = pl->borders;
        ca.P = c->P;
        ca.cfo_out = cfo;
        ca.count = d_cnt;  // single batch when set (f0 == 0)
        StreamParamsArgs sa{};
        sa.tab = c->tables(true);
        sa.iq = reinterpret_cast<const double2*>(a.iq);
        sa.iq16 = reinterpret_cast<const short2*>(a.iq16);
        sa.starts = d_list + f0;
        sa.nframes = (long)nb;
        sa.cfo = cfo;
        sa.pre = c->d_preamble;
        sa.mod_pre = c->d_modpre;
        sa.chan_out = chan;  // internal scratch: reciprocals for rx's multiply
        sa.chan_recip = true;
        sa.corr_out = corr;
        sa.npr = c->npr;
        sa.S = c->S;
        sa.D = c->D;
        sa.P = c->P;
        sa.cp = c->cp;
        sa.pilot_ampl = (double)c->p.pilot_ampl / 1000;
        sa.count = d_cnt;
        // (dec_tau / dec_fast stay unset: the stream rx keeps the arithmetic emit)
        RxArgs ra{};
        ra.tab = c->tables(false);
        ra.iq = reinterpret_cast<const double2*>(a.iq);
        ra.iq16 = reinterpret_cast<const short2*>(a.iq16);
        ra.nframes = (long)nb;
        ra.starts = d_list + f0;
        ra.start_off = preamble_len(c) + c->cp;
        ra.count = d_cnt;
        ra.corr = corr;
        ra.chan = chan;
        ra.chan_stride = c->D;
        ra.chan_recip = true;
        ra.constell = a.constell_out ? reinterpret_cast<double2*>(a.constell_out) + f0 * d.npts : nullptr;
        ra.bytes = a.bytes_out ? a.bytes_out + f0 * c->geo.bytes_per_frame : nullptr;
        ra.S = c->S;
        ra.D = c->D;
        ra.P = c->P;
        ra.seg = c->seg;
        ra.cp = c->cp;
        ra.k = c->k;
        ra.bytes_per_frame = c->geo.bytes_per_frame;
        ra.pilot_ampl = (double)c->p.pilot_ampl / 1000;
        // static frame order: the next frame's symbol 0 is fetched ahead of
        // the gains (stream rx 500 -> 416 us with the queue's late fetch)
        ra.queue = nullptr;
        // One kernel for the whole decode where the geometry allows (N =
        // 512, 640-point CFO form: sync stage + rx stage per frame, the
        // ramps and channel through LDS); else pilot_freq_sinh + the
        // params stage (one kernel or two), then the stream rx.
        hipError_t e2 = c->walk.staged_decode ? hipErrorNotSupported
                                              : launch_stream_decode(ca, sa, ra, c->logn, pl->logm, pl->g, d.st);
        if (e2 == hipErrorNotSupported) {
            // other geometries: pilot_freq_sinh, the params stage, then
            // the stream rx (two waves per frame at N = 512)
            e2 = launch_cfo(pl->logm, pl->g, ca, d.st);
            if (e2 != hipSuccess) return hip_fail(e2, "stream cfo launch");
            e2 = launch_stream_params(c->logn, sa, d.st);
            if (e2 != hipSuccess) return hip_fail(e2, "stream params launch");
            e2 = launch_rx(c->logn, ra, d.st, nullptr);
            if (e2 != hipSuccess) return hip_fail(e2, "stream rx launch");
        } else if (e2 != hipSuccess) {
            return hip_fail(e2, "stream decode launch");
        }
    }
    return OFDM_OK;
}

// Geometries the fused kernels do not take: gather each frame of d_list
// into a batch, then the staged sync chain + demod
int decode_gathered(const Decode& d, const long* d_list, size_t nout)
{
    ofdm_ctx* c = d.c;
    const StreamCall& a = *d.a;
    const long pre = preamble_len(c), span = pre + message_len(c);
    const size_t fb = (size_t)span * sizeof(double2);
    const size_t bmax = std::min<size_t>(65535, batch_frames(fb, d.batch_cap));
    const size_t nb0 = std::min(nout, bmax);
    int r2;
    if ((r2 = grow(c, c->s_batch, nb0 * fb)) || (r2 = grow(c, c->s_chan, nb0 * c->D * sizeof(double2)))) return r2;
    double* batch = static_cast<double*>(c->s_batch.p.get());
    double* chan = static_cast<double*>(c->s_chan.p.get());
    for (size_t f0 = 0; f0 < nout; f0 += nb0) {
        const size_t nb = std::min(nb0, nout - f0);
        GatherArgs ga{reinterpret_cast<const double2*>(a.iq), reinterpret_cast<const short2*>(a.iq16), (long)a.n,
                      d_list + f0, (long)nb, span, reinterpret_cast<double2*>(batch)};
        hipError_t e2 = launch_gather(ga, d.st);
        if (e2 != hipSuccess) return hip_fail(e2, "gather launch");
        if ((r2 = ofdm_sync_frames(c, batch, nb, (size_t)span, OFDM_SYNC_ALL, nullptr,
                                   a.cfo_out ? a.cfo_out + f0 : nullptr, chan, a.stream)))
            return r2;
        if ((r2 = ofdm_rx_demod(c, batch + 2 * pre, nb, (size_t)span, chan, (size_t)c->D,
                                a.constell_out ? a.constell_out + 2 * f0 * d.npts : nullptr,
                                a.bytes_out ? a.bytes_out + f0 * c->geo.bytes_per_frame : nullptr, nullptr, nullptr,
                                a.stream)))
            return r2;
    }
    return OFDM_OK;
}

// A known list of `nout` frames, the first `neg` of them before sample 0 (a
// prefix; the fused kernels skip them): those take the gather path, whose
// samples before 0 read as zero like rx.cpp's header
int decode_list(const Decode& d, const long* d_list, size_t nout, size_t neg)
{
    if (!d.fused) return decode_gathered(d, d_list, nout);
    if (int rc = decode_fused(d, d_list, nout, nullptr)) return rc;
    return neg ? decode_gathered(d, d_list, neg) : OFDM_OK;
}

// The resolve kernel's last word is the flags word of the status: poll it
// (no event between the resolve and the decode: a marker between two
// dependent kernels costs a launch gap); if it has not landed in 2 s, wait
// for the stream (errors surface there)
int wait_status(volatile long* hs, hipStream_t st)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (long spin = 0; hs[1] == -1; ++spin)
        if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            HIP_TRY(hipStreamSynchronize(st));
            break;
        }
    return OFDM_OK;
}

// the true walk's records (the resolve kernel's chain) into the caller's arrays
int read_chain(ofdm_ctx* c, const StreamCall& a, size_t nchain)
{
    const size_t nl = std::min(nchain, a.located_cap);
    if (!nl) return OFDM_OK;
    std::vector<long> rl(nl);
    HIP_TRY(hipMemcpy(rl.data(), c->s_chain.p, nl * sizeof(long), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nl; ++i) {
        if (a.located) a.located[i] = rec_pb(rl[i]);
        if (a.located_lag) a.located_lag[i] = rec_lag(rl[i]) ? 1 : 0;
    }
    return OFDM_OK;
}

// The look-back walk's finish. The true walk, resolved on the device: the
// owned frames straight into the decode's list (and pb_out), a status block
// to the host. The decode is enqueued behind it before the host reads the
// status. *overflow: a walker's records overflowed and nothing was written;
// the caller takes the halo walk.
int finish_lookback(ofdm_ctx* c, const StreamCall& a, const Walk& wk, const Decode& dec, bool debug, bool* overflow)
{
    const WalkPlan& p = wk.plan;
    hipStream_t st = dec.st;
    int rc;
    const size_t ub = std::min(a.max_frames, (size_t)p.nchunks * p.max_rec);
    const bool want_chain = (a.located || a.located_lag) && a.located_cap > 0;
    const size_t chain_tail = a.located_cap / 2, chain_head = a.located_cap - chain_tail;
    if ((rc = grow(c, c->s_pbs, (ub + 1) * sizeof(long))) || (rc = grow_host(c, c->h_status, 64)) ||
        (want_chain && (rc = grow(c, c->s_chain, a.located_cap * sizeof(long)))))
        return rc;
    long* d_pbs = static_cast<long*>(c->s_pbs.p.get());
    volatile long* hs = static_cast<volatile long*>(c->h_status.p.get());
    hs[1] = -1;  // overwritten by the resolve kernel
    ResolveArgs ra{};
    ra.rec = wk.dev.rec;
    ra.nrec = wk.dev.nrec;
    ra.link = wk.dev.link;
    ra.exit_pos = wk.dev.exit_pos;
    ra.exit_ring = wk.dev.exit_ring;
    ra.nchunks = p.nchunks;
    ra.max_rec = p.max_rec;
    // a core starting at the stream's first sample also owns a frame whose
    // preamble starts before it (rx.cpp:105-114,158: its zero header)
    ra.own_lo = a.own_lo == 0 ? LONG_MIN : a.own_lo;
    ra.own_hi = a.own_hi;
    ra.cap = (long)ub;
    ra.list = d_pbs;
    ra.list2 = a.pb_out;
    ra.count = d_pbs + ub;
    ra.chain = want_chain ? static_cast<long*>(c->s_chain.p.get()) : nullptr;
    ra.chain_head = (long)chain_head;
    ra.chain_tail = (long)chain_tail;
    ra.status = const_cast<long*>(hs);
    ra.pub = wk.args.pub;
    ra.queue_reset = c->d_queue;
    hipError_t e = launch_resolve(ra, st);
    if (e != hipSuccess) return hip_fail(e, "stream resolve launch");
    c->pub_zero = true;    // cleared by the resolve (stream order)
    c->queue_zero = true;  // likewise the chunk counter
    if (wk.timed) HIP_TRY(hipEventRecord(c->ev_phase[2], st));
    const bool spec = speculative_ok(dec, ub);
    if (spec && (rc = decode_fused(dec, d_pbs, ub, d_pbs + ub))) return rc;
    if (wk.timed && spec) {
        HIP_TRY(hipEventRecord(c->ev_phase[3], st));
        c->phase_valid = true;
    }
    if ((rc = wait_status(hs, st))) return rc;
    const long owned = hs[0], flags = hs[1], xpos = hs[2], xring = hs[3], nchain = hs[4], nneg = hs[5];
    if (flags < 0) return fail(OFDM_ERR_HIP, "stream resolve wrote no status");
    if (flags & RESOLVE_OVERFLOW) {
        // a walker's records overflowed (a walk that met no later chunk's
        // through a whole core): the halo walk with host stitching
        if (debug) fprintf(stderr, "ofdm_rx_stream: look-back overflow, halo walk\n");
        *overflow = true;
        return OFDM_OK;
    }
    *a.nframes_out = (size_t)owned;
    if (a.exit_out) *a.exit_out = ofdm_walk_state{xpos, xpos < 0 ? 0 : xring};
    if (a.nlocated_out) *a.nlocated_out = (size_t)nchain;
    if (want_chain && (rc = read_chain(c, a, (size_t)nchain))) return rc;
    if (debug)
        fprintf(stderr, "ofdm_rx_stream: look-back, %ld chunks of %ld samples, halo %ld, %ld frames\n", p.nchunks,
                p.chunk, p.halo, owned);
    const size_t nout = std::min((size_t)owned, ub);
    // frames before sample 0 (a prefix; the fused kernels skip them): the
    // gather path, whose samples before 0 read as zero like rx.cpp's header
    const size_t neg = (flags & RESOLVE_NEG_FRAME) ? std::min((size_t)nneg, nout) : 0;
    if (spec) return neg ? decode_gathered(dec, d_pbs, neg) : OFDM_OK;
    if (nout == 0) return OFDM_OK;
    return decode_list(dec, d_pbs, nout, neg);
}

// Every chunk's in-core records, compacted on the device behind the walk into
// s_pbs (and pb_out): the speculative list of up to ub frames, its count
// behind it
int launch_compaction(ofdm_ctx* c, const StreamCall& a, const Walk& wk, size_t ub, hipStream_t st)
{
    if (int rc = grow(c, c->s_pbs, (ub + 1) * sizeof(long))) return rc;
    long* d_pbs = static_cast<long*>(c->s_pbs.p.get());
    CompactArgs ka{};
    ka.rec = wk.dev.rec;
    ka.ncore = wk.dev.ncore;
    ka.first_in = wk.dev.first_in;
    ka.nchunks = wk.plan.nchunks;
    ka.max_rec = wk.plan.max_rec;
    ka.cap = (long)ub;
    ka.list = d_pbs;
    ka.list2 = a.pb_out;
    ka.count = d_pbs + ub;
    ka.queue_reset = c->d_queue;  // after the walk (stream order): zero for the next call
    hipError_t e = launch_compact(ka, st);
    if (e != hipSuccess) return hip_fail(e, "stream compact launch");
    return OFDM_OK;
}

// Chunk k again from the exact state (pos, ring_end), with one workgroup; its
// row of the host mirror `h` is refreshed when this returns
int rewalk_chunk(ofdm_ctx* c, const Walk& wk, const WalkView& h, long k, long pos, long ring_end, hipStream_t st)
{
    const WalkView& d = wk.dev;
    const int max_rec = wk.plan.max_rec;
    WalkArgs r = wk.args;
    const int id = (int)k;
    const long st2[2] = {pos, ring_end};
    HIP_TRY(hipMemcpyAsync(d.start, st2, sizeof(st2), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d.ids, &id, sizeof(int), hipMemcpyHostToDevice, st));
    r.start_pos = d.start;
    r.start_ring = d.start + 1;
    r.chunk_ids = d.ids;
    r.queue = nullptr;
    hipError_t e2 = launch_stream_walk(c->t2_logn, r, 1, st);
    if (e2 != hipSuccess) return hip_fail(e2, "stream_walk re-walk launch");
    HIP_TRY(hipMemcpyAsync(h.rec + (size_t)k * max_rec, d.rec + (size_t)k * max_rec, max_rec * sizeof(long),
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h.exit_pos[k], d.exit_pos + k, sizeof(long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h.exit_ring[k], d.exit_ring + k, sizeof(long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h.nrec[k], d.nrec + k, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return OFDM_OK;
}

void print_rewalk(const WalkTable& t, const Stitched& s, const StreamCall& a, long chunk, long k, long pos,
                  long ring_end)
{
    long lo, hi;
    chunk_core(k, a.own_lo, a.own_hi, chunk, lo, hi);
    fprintf(stderr, "ofdm_rx_stream: re-walk chunk %ld [%ld, %ld) from (%ld, %ld); its walk:", k, lo, hi, pos, ring_end);
    for (int i = 0; i < t.nrec[k]; ++i) {
        const long r = t.rec[(size_t)k * t.max_rec + i];
        fprintf(stderr, " %ld%s", rec_pb(r), rec_lag(r) ? "+" : "");
    }
    fprintf(stderr, " | previous:");
    for (long r : s.last) fprintf(stderr, " %ld%s", rec_pb(r), rec_lag(r) ? "+" : "");
    fprintf(stderr, "\n");
}

// the shard report of the stitched walk: nlocated and the located arrays
void report_located(const StreamCall& a, const Stitched& s)
{
    if (!a.nlocated_out) return;
    std::vector<long> all;
    *a.nlocated_out = located_list(s, a.own_hi, a.located_cap, all);
    for (size_t i = 0; i < all.size(); ++i) {
        if (a.located) a.located[i] = rec_pb(all[i]);
        if (a.located_lag) a.located_lag[i] = rec_lag(all[i]) ? 1 : 0;
    }
}

// The stitched walk's frames to the device (s_pbs, pb_out), then their decode:
// located frames -> main.cpp:60-80 chain + demod
int decode_stitched(ofdm_ctx* c, const StreamCall& a, const Decode& dec, const std::vector<long>& frames, size_t ub)
{
    hipStream_t st = dec.st;
    const size_t nout = std::min(frames.size(), a.max_frames);
    int rc;
    if ((rc = grow(c, c->s_pbs, (std::max(nout, ub) + 1) * sizeof(long))) ||
        (rc = grow_host(c, c->h_frames, nout * sizeof(long))))
        return rc;
    long* d_pbs = static_cast<long*>(c->s_pbs.p.get());
    // the previous call's copy out of the pinned stage must have finished: on
    // the same stream the walk-record sync before the stitch saw to it
    if (c->h_frames_used && c->h_frames_stream != st) HIP_TRY(hipStreamSynchronize(c->h_frames_stream));
    c->h_frames_stream = st;
    c->h_frames_used = true;
    std::memcpy(c->h_frames.p, frames.data(), nout * sizeof(long));
    HIP_TRY(hipMemcpyAsync(d_pbs, c->h_frames.p, nout * sizeof(long), hipMemcpyHostToDevice, st));
    if (a.pb_out) HIP_TRY(hipMemcpyAsync(a.pb_out, d_pbs, nout * sizeof(long), hipMemcpyDeviceToDevice, st));
    size_t neg = 0;  // frames before sample 0: the gather path (the fused kernels skip them)
    while (neg < nout && frames[neg] < 0) ++neg;
    return decode_list(dec, d_pbs, nout, neg);
}

// The halo walk's finish: the walk records to the host, the chunk walks
// stitched there (ofdm_stream_stitch.hpp), then the decode of the stitched
// walk's frames, unless the speculative decode already was that.
int finish_halo(ofdm_ctx* c, const StreamCall& a, const Walk& wk, const Decode& dec, bool debug)
{
    const WalkPlan& p = wk.plan;
    hipStream_t st = dec.st;
    int rc;
    // records, exit states and counts in one copy of the walk buffer's layout
    if ((rc = grow_host(c, c->h_walk, wk.buf.host_bytes()))) return rc;
    const WalkView host = wk.buf.view(c->h_walk.p);
    if (!c->ev_walk) HIP_TRY(hipEventCreateWithFlags(c->ev_walk.put(), hipEventDisableTiming));
    if (!c->ev_wdone) HIP_TRY(hipEventCreateWithFlags(c->ev_wdone.put(), hipEventDisableTiming));
    if (!c->side) HIP_TRY(hipStreamCreateWithFlags(c->side.put(), hipStreamNonBlocking));
    // Speculative decode: every chunk's in-core records, compacted on the
    // device behind the walk, are decoded while the host stitches the walks.
    // That list is the stitched walk unless a chunk needs a re-walk (or the
    // walk ends early); then the host's list is decoded again over it.
    const size_t ub = std::min(a.max_frames, (size_t)p.nchunks * p.max_rec);
    const bool spec = speculative_ok(dec, ub);
    if (spec && (rc = launch_compaction(c, a, wk, ub, st))) return rc;
    // The walk records go to the host on a side stream, so the decode on the
    // caller's stream does not queue behind the copy. The one event marks the
    // walk and the compaction together: a marker between two dependent
    // kernels costs a launch gap, so walk -> compaction runs back to back.
    HIP_TRY(hipEventRecord(c->ev_wdone, st));
    HIP_TRY(hipStreamWaitEvent(c->side, c->ev_wdone, 0));
    HIP_TRY(hipMemcpyAsync(host.rec, wk.dev.rec, wk.buf.host_bytes(), hipMemcpyDeviceToHost, c->side));
    HIP_TRY(hipEventRecord(c->ev_walk, c->side));
    if (spec) {
        const long* d_pbs = static_cast<const long*>(c->s_pbs.p.get());
        if ((rc = decode_fused(dec, d_pbs, ub, d_pbs + ub))) return rc;
        // the queue counter was zeroed by the compaction (stream order)
        c->queue_zero = true;
    }
    HIP_TRY(hipEventSynchronize(c->ev_walk));

    const WalkTable tab{host.rec, host.nrec, host.exit_pos, host.exit_ring, p.nchunks, p.max_rec};
    // the speculative list, from the walks as they came back
    std::vector<long> spec_frames;
    if (spec) spec_frames = spec_list(tab, a.own_lo, a.own_hi, p.chunk);
    Stitched s;
    auto rewalk = [&](long k, long pos, long ring_end) -> int {
        if (debug) print_rewalk(tab, s, a, p.chunk, k, pos, ring_end);
        return rewalk_chunk(c, wk, host, k, pos, ring_end, st);
    };
    rc = stitch_chunks(tab, a.own_lo, a.own_hi, p.chunk, a.start.ring_end, rewalk, s);
    if (rc == STITCH_OVERFLOW) return fail(OFDM_ERR_HIP, "stream walk record overflow");
    if (rc) return rc;
    *a.nframes_out = s.frames.size();
    if (a.exit_out && s.has_exit) *a.exit_out = ofdm_walk_state{s.exit_pos, s.exit_ring};
    report_located(a, s);
    const bool hit = spec && s.frames == spec_frames;  // the speculative decode was the true one
    if (debug)
        fprintf(stderr, "ofdm_rx_stream: %ld chunks of %ld samples, halo %ld, %ld re-walks, %zu frames, speculative %s\n",
                p.nchunks, p.chunk, p.halo, s.nrewalk, s.frames.size(), spec ? (hit ? "hit" : "miss") : "off");
    if (hit || s.frames.empty() || a.max_frames == 0) return OFDM_OK;
    return decode_stitched(c, a, dec, s.frames, ub);
}

// One attempt at the call under `plan`: scratch, ordering, the walk, and the
// plan's finish
int run_walk(ofdm_ctx* c, const StreamCall& a, const WalkPlan& plan, bool debug, size_t batch_cap, bool* overflow)
{
    hipStream_t st = (hipStream_t)a.stream;
    Walk wk(plan);
    int rc;
    if ((rc = grow(c, c->s_walk, wk.buf.device_bytes()))) return rc;
    wk.dev = wk.buf.view(c->s_walk.p);
    if ((rc = fill_walk_args(c, a, plan, wk.dev, wk.args)) || (rc = order_after_previous_call(c, st)) ||
        (rc = launch_walk(c, wk, st)))
        return rc;
    const Decode dec = decode_backend(c, a, st, batch_cap);
    return plan.lbk ? finish_lookback(c, a, wk, dec, debug, overflow) : finish_halo(c, a, wk, dec, debug);
}

}  // namespace

int rx_stream_call(ofdm_ctx* c, const StreamCall& a)
{
    int rc = check_stream_call(c, a);
    if (rc) return rc;
    if (a.n == 0 || a.start.pos >= (long)a.n) return OFDM_OK;
    const bool debug = stream_debug();
    const size_t batch_cap = decode_batch_cap();
    WalkPlan plan;
    bool overflow = false;
    if ((rc = plan_walk(c, a, a.chunk, false, &plan)) || (rc = run_walk(c, a, plan, debug, batch_cap, &overflow)))
        return rc;
    if (!overflow) return OFDM_OK;
    // a look-back walker's records overflowed: the whole call again as the
    // halo walk, over the same chunks
    if ((rc = plan_walk(c, a, plan.chunk, true, &plan))) return rc;
    return run_walk(c, a, plan, debug, batch_cap, &overflow);
}

}  // namespace ofdm
