// ofdm_stream_stitch.hpp — the host's list logic of the stream receiver's halo
// walk (ofdm_stream_call.cpp): what a walk record holds, the stitch of the
// chunk walks into the one true walk, the located list of a shard report and
// the speculative list. Plain C++ with no HIP in it, so that
// apps/stitch_selftest.cpp tests it without a GPU.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <vector>

namespace ofdm {

// A walk record (ofdm_sync.hpp, WALK_REC_LAG / WALK_REC_PB, equal to these by
// a static_assert in ofdm_stream_call.cpp): a preamble start, plus bit 62 in
// ring mode when the state after the frame has the later of its two ring ends
constexpr long REC_LAG_BIT = 1L << 62;
constexpr long REC_PB_MASK = REC_LAG_BIT - 1;

// a record's preamble start (ring mode: the lag bit stripped; a frame before
// the stream's first sample stays negative)
inline long rec_pb(long r) { return r < 0 ? r : (r & REC_PB_MASK); }
inline bool rec_lag(long r) { return r > 0 && (r & REC_LAG_BIT); }

// The walkers' results as the host sees them: chunk k's records are
// rec[k * max_rec .. + nrec[k]) (nrec[k] > max_rec: they overflowed), its walk
// left off in state (exit_pos[k], exit_ring[k]); exit_pos[k] < 0: the stream
// was exhausted
struct WalkTable {
    long* rec;
    int* nrec;
    long* exit_pos;
    long* exit_ring;
    long nchunks;
    int max_rec;
};

struct Stitched {
    std::vector<long> frames;     // preamble starts of the owned frames, in walk order
    std::vector<long> walk_in;    // records of the frames chunk 0 located before own_lo
    std::vector<long> owned_rec;  // the owned frames' records
    std::vector<long> last;       // every record of the last accepted chunk's walk
    long last_k = -1;             // that chunk (< nchunks - 1: the true walk ended early)
    bool has_exit = false;        // the walk passed every chunk: (exit_pos, exit_ring) is its state
    long exit_pos = 0, exit_ring = 0;
    long nrewalk = 0;
};

constexpr int STITCH_OVERFLOW = INT_MIN;  // a chunk's count exceeds max_rec (no status of a re-walk is this)

// the cores tile [own_lo, own_hi): chunk k owns [lo, hi)
inline void chunk_core(long k, long own_lo, long own_hi, long chunk, long& lo, long& hi)
{
    lo = own_lo + k * chunk;
    hi = std::min(lo + chunk, own_hi);
}

// Stitch the chunk walks into the one true walk. Chunk 0 starts at the true
// initial state. Chunk k is accepted when its walk and the accepted walk
// before it locate a common frame no later than k's first owned frame (from
// there on both are the same computation); otherwise rewalk(k, pos, ring_end)
// walks it again from the previous exit state (exact) and refreshes its row
// of the table; a status other than 0 ends the stitch and is returned.
// Records compare whole (preamble start and, in ring mode, the ring of the
// state after the frame): equal records = equal walks from there on.
// While rewalk runs, out.last still holds the previous accepted walk.
template <class Rewalk>
int stitch_chunks(const WalkTable& t, long own_lo, long own_hi, long chunk, long start_ring_end, Rewalk&& rewalk,
                  Stitched& out)
{
    out = Stitched{};
    std::vector<long>& prev = out.last;
    long texit = 0, texit_ring = start_ring_end;
    for (long k = 0; k < t.nchunks; ++k) {
        if (k > 0 && texit < 0) break;  // the true walk ended
        if (t.nrec[k] > t.max_rec) return STITCH_OVERFLOW;
        const long* row = t.rec + (size_t)k * t.max_rec;
        std::vector<long> lst(row, row + t.nrec[k]);
        long lo, hi;
        chunk_core(k, own_lo, own_hi, chunk, lo, hi);
        if (k > 0) {
            long first_owned = LONG_MAX;
            for (long r : lst)
                if (rec_pb(r) >= lo && rec_pb(r) < hi) first_owned = std::min(first_owned, rec_pb(r));
            bool sync = false;
            for (long r : lst)
                if (rec_pb(r) <= first_owned && std::find(prev.begin(), prev.end(), r) != prev.end()) sync = true;
            if (!sync) {
                ++out.nrewalk;
                if (int rc = rewalk(k, texit, texit_ring)) return rc;
                if (t.nrec[k] > t.max_rec) return STITCH_OVERFLOW;
                lst.assign(row, row + t.nrec[k]);
            }
        }
        if (k == 0)  // the walk-in from the start state (true by definition): frames before own_lo; a
            for (long r : lst) {  // core from sample 0 owns a frame before it (rx.cpp's zero header)
                if (rec_pb(r) < lo && !(own_lo == 0 && r < 0)) out.walk_in.push_back(r);
                if (own_lo == 0 && r < 0) {
                    out.frames.push_back(r);
                    out.owned_rec.push_back(r);
                }
            }
        for (long r : lst)
            if (rec_pb(r) >= lo && rec_pb(r) < hi) {
                out.frames.push_back(rec_pb(r));
                out.owned_rec.push_back(r);
            }
        prev.swap(lst);
        texit = t.exit_pos[k];
        texit_ring = t.exit_ring[k];
        out.last_k = k;
    }
    out.has_exit = out.last_k == t.nchunks - 1;
    out.exit_pos = texit;
    out.exit_ring = texit < 0 ? 0 : texit_ring;
    return 0;
}

// Every frame of the stitched walk: the walk-in, the owned frames, and what
// the last walker located past own_hi before it stopped. Returns how many
// they are; `out` holds their records, or, when they are more than cap, the
// first cap - cap/2 and the last cap/2 of them.
inline size_t located_list(const Stitched& s, long own_hi, size_t cap, std::vector<long>& out)
{
    out = s.walk_in;
    out.insert(out.end(), s.owned_rec.begin(), s.owned_rec.end());
    if (s.has_exit)
        for (long r : s.last)
            if (rec_pb(r) >= own_hi) out.push_back(r);
    const size_t n = out.size();
    if (n > cap) {
        const size_t tail = cap / 2, head = cap - tail;
        out.erase(out.begin() + head, out.end() - tail);
    }
    return n;
}

// The list the speculative decode took, from the walks as they came back:
// every chunk's records inside its own core, in chunk order (CompactArgs)
inline std::vector<long> spec_list(const WalkTable& t, long own_lo, long own_hi, long chunk)
{
    std::vector<long> out;
    for (long k = 0; k < t.nchunks; ++k) {
        long lo, hi;
        chunk_core(k, own_lo, own_hi, chunk, lo, hi);
        for (int i = 0; i < std::min(t.nrec[k], t.max_rec); ++i) {
            const long pb = rec_pb(t.rec[(size_t)k * t.max_rec + i]);
            if (pb >= lo && pb < hi) out.push_back(pb);
        }
    }
    return out;
}

}  // namespace ofdm
