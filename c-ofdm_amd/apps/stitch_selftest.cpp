// stitch_selftest — the stream receiver's host stitch (csrc/ofdm_stream_stitch.hpp)
// on hand-written walk tables: no GPU, no library. Exit status 0: every check held.
#include <cstdio>
#include <utility>
#include <vector>

#include "../csrc/ofdm_stream_stitch.hpp"

using namespace ofdm;
using V = std::vector<long>;

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

// a walk table of `rows.size()` chunks; chunk k exits in state (ex[k], exr[k])
struct Table {
    int max_rec;
    V rec, ex, exr;
    std::vector<int> nrec;
    Table(int max_rec_, const std::vector<V>& rows, V ex_, V exr_)
        : max_rec(max_rec_), rec(rows.size() * max_rec_, -999), ex(std::move(ex_)), exr(std::move(exr_)),
          nrec(rows.size())
    {
        for (size_t k = 0; k < rows.size(); ++k) set(k, rows[k]);
    }
    void set(size_t k, const V& row)
    {
        nrec[k] = (int)row.size();
        for (size_t i = 0; i < row.size() && i < (size_t)max_rec; ++i) rec[k * max_rec + i] = row[i];
    }
    WalkTable view() { return WalkTable{rec.data(), nrec.data(), ex.data(), exr.data(), (long)nrec.size(), max_rec}; }
};

struct Call {
    long k, pos, ring_end;
};
static const auto no_rewalk = [](long, long, long) {
    CHECK(!"re-walk of a chunk that shares a record");
    return 1;
};

// cores of 100 samples from own_lo = 100: [100, 200), [200, 300), [300, 400)
static const long LAG = REC_LAG_BIT;

static void records()
{
    CHECK(rec_pb(210) == 210 && rec_pb(210 | LAG) == 210 && rec_pb(-30) == -30 && rec_pb(0) == 0);
    CHECK(!rec_lag(210) && rec_lag(210 | LAG) && !rec_lag(-30) && !rec_lag(0));
}

static void case_a_every_chunk_shares()
{
    Table t(5, {{50, 120, 180 | LAG, 210}, {180 | LAG, 210, 260, 310}, {260, 310, 350, 420}}, {215, 315, 425},
            {7, 8, 9});
    Stitched s;
    CHECK(stitch_chunks(t.view(), 100, 400, 100, 3, no_rewalk, s) == 0);
    CHECK((s.frames == V{120, 180, 210, 260, 310, 350}));
    CHECK((s.owned_rec == V{120, 180 | LAG, 210, 260, 310, 350}));
    CHECK((s.walk_in == V{50}));
    CHECK((s.last == V{260, 310, 350, 420}));
    CHECK(s.nrewalk == 0 && s.last_k == 2 && s.has_exit && s.exit_pos == 425 && s.exit_ring == 9);
    // the speculative list of the same table: every chunk's in-core records
    CHECK((spec_list(t.view(), 100, 400, 100) == V{120, 180, 210, 260, 310, 350}));
    // a single chunk: nothing to stitch
    Table one(4, {{130, 160}}, {170}, {0});
    CHECK(stitch_chunks(one.view(), 100, 200, 100, 0, no_rewalk, s) == 0);
    CHECK((s.frames == V{130, 160}) && s.has_exit && s.last_k == 0 && s.exit_pos == 170);
}

static void case_b_no_shared_record()
{
    Table t(5, {{50, 120, 180, 210}, {205, 265}, {260, 310, 350}}, {215, 270, 360}, {7, 8, 9});
    CHECK((spec_list(t.view(), 100, 400, 100) == V{120, 180, 205, 265, 310, 350}));  // as the walks came back
    std::vector<Call> calls;
    Stitched s;
    auto rewalk = [&](long k, long pos, long ring_end) {
        calls.push_back({k, pos, ring_end});
        CHECK((s.last == V{50, 120, 180, 210}));  // the previous accepted walk, while the re-walk runs
        t.set(1, {260, 310});
        t.ex[1] = 312;
        t.exr[1] = 18;
        return 0;
    };
    CHECK(stitch_chunks(t.view(), 100, 400, 100, 3, rewalk, s) == 0);
    CHECK(calls.size() == 1 && calls[0].k == 1 && calls[0].pos == 215 && calls[0].ring_end == 7);
    // the refreshed row is the one used: for the frames (no 205 or 265; 210 lies before the re-walk's
    // start), and as chunk 2's predecessor (260 is shared: no second re-walk)
    CHECK((s.frames == V{120, 180, 260, 310, 350}));
    CHECK(s.nrewalk == 1 && s.has_exit && s.exit_pos == 360 && s.exit_ring == 9);
    // a re-walk's status other than 0 ends the stitch and is returned
    auto refuse = [&](long, long, long) { return 42; };
    Table t2(5, {{120}, {230}, {330}}, {130, 240, 340}, {0, 0, 0});
    CHECK(stitch_chunks(t2.view(), 100, 400, 100, 3, refuse, s) == 42);
}

static void case_c_shared_record_after_first_owned()
{
    Table t(5, {{120, 180, 210}, {205, 210, 260}, {260, 310}}, {215, 270, 320}, {0, 0, 0});
    int calls = 0;
    Stitched s;
    auto rewalk = [&](long k, long pos, long) {
        ++calls;
        CHECK(k == 1 && pos == 215);
        t.set(1, {210, 260});
        return 0;
    };
    CHECK(stitch_chunks(t.view(), 100, 400, 100, 0, rewalk, s) == 0);
    CHECK(calls == 1 && s.nrewalk == 1);
    CHECK((s.frames == V{120, 180, 210, 260, 310}));
    // shared at the first owned frame itself: accepted
    Table u(5, {{120, 180, 210}, {210, 260}, {260, 310}}, {215, 270, 320}, {0, 0, 0});
    CHECK(stitch_chunks(u.view(), 100, 400, 100, 0, no_rewalk, s) == 0);
    CHECK((s.frames == V{120, 180, 210, 260, 310}));
}

static void case_d_lag_bit_differs()
{
    Table t(5, {{120, 180, 210 | LAG}, {210, 260}, {260, 310}}, {215, 270, 320}, {5, 6, 7});
    int calls = 0;
    Stitched s;
    auto rewalk = [&](long k, long pos, long ring_end) {
        ++calls;
        CHECK(k == 1 && pos == 215 && ring_end == 5);
        t.set(1, {210 | LAG, 260});
        return 0;
    };
    CHECK(stitch_chunks(t.view(), 100, 400, 100, 0, rewalk, s) == 0);
    CHECK(calls == 1);
    CHECK((s.frames == V{120, 180, 210, 260, 310}));
    CHECK((s.owned_rec == V{120, 180, 210 | LAG, 260, 310}));
}

static void case_e_walk_ends_early()
{
    Table t(5, {{120, 180}, {180, 230}, {230, 330}, {330, 430}}, {190, -1, 340, 440}, {4, 5, 6, 7});
    Stitched s;
    CHECK(stitch_chunks(t.view(), 100, 500, 100, 0, no_rewalk, s) == 0);
    CHECK((s.frames == V{120, 180, 230}));
    CHECK(s.last_k == 1 && s.last_k < 3 && !s.has_exit);
    CHECK((s.last == V{180, 230}));
    V all;
    CHECK(located_list(s, 500, 16, all) == 3 && (all == V{120, 180, 230}));  // nothing past own_hi without an exit
    // the stream exhausted by the last chunk: an exit state with no ring end
    Table u(5, {{120, 180}, {180, 230}}, {190, -1}, {4, 5});
    CHECK(stitch_chunks(u.view(), 100, 300, 100, 0, no_rewalk, s) == 0);
    CHECK(s.has_exit && s.exit_pos == -1 && s.exit_ring == 0);
}

static void case_f_frame_before_sample_0()
{
    Table t(5, {{-30, 40, 90}, {90, 140}, {140, 250}}, {95, 150, 260}, {0, 0, 0});
    Stitched s;
    CHECK(stitch_chunks(t.view(), 0, 300, 100, 0, no_rewalk, s) == 0);
    CHECK((s.frames == V{-30, 40, 90, 140, 250}) && (s.owned_rec == s.frames) && s.walk_in.empty());
    Table u(5, {{-30, 40, 120}, {120, 240}, {240, 310}}, {130, 250, 320}, {0, 0, 0});
    CHECK(stitch_chunks(u.view(), 100, 400, 100, 0, no_rewalk, s) == 0);
    CHECK((s.walk_in == V{-30, 40}) && (s.frames == V{120, 240, 310}));
}

static void case_g_record_overflow()
{
    Table t(4, {{120, 180}, {180, 230, 240, 250, 260}, {260, 330}}, {190, 270, 340}, {0, 0, 0});
    Stitched s;
    CHECK(stitch_chunks(t.view(), 100, 400, 100, 0, no_rewalk, s) == STITCH_OVERFLOW);
    Table u(4, {{120, 180}, {230}, {230, 330}}, {190, 240, 340}, {0, 0, 0});
    int calls = 0;
    auto rewalk = [&](long, long, long) {
        ++calls;
        u.nrec[1] = 5;  // the re-walk's records overflowed
        return 0;
    };
    CHECK(stitch_chunks(u.view(), 100, 400, 100, 0, rewalk, s) == STITCH_OVERFLOW);
    CHECK(calls == 1);
    // a count of exactly max_rec is no overflow
    Table v(4, {{120, 150, 170, 180}, {180, 230}, {230, 330}}, {190, 240, 340}, {0, 0, 0});
    CHECK(stitch_chunks(v.view(), 100, 400, 100, 0, no_rewalk, s) == 0);
    // the speculative list reads at most max_rec records of an overflowed row
    CHECK((spec_list(t.view(), 100, 400, 100) == V{120, 180, 230, 240, 250, 330}));
}

static void case_h_located_list()
{
    Stitched s;
    s.walk_in = {10, 60};
    s.owned_rec = {120, 180 | LAG, 210, 260, 350};
    s.last = {260, 350, 420 | LAG, 480};
    s.has_exit = true;
    const V full = {10, 60, 120, 180 | LAG, 210, 260, 350, 420 | LAG, 480};
    V all;
    CHECK(located_list(s, 400, 7, all) == 9);
    CHECK((all == V{10, 60, 120, 180 | LAG, 350, 420 | LAG, 480}));  // the first 4, the last 3
    CHECK(located_list(s, 400, 0, all) == 9 && all.empty());
    CHECK(located_list(s, 400, 9, all) == 9 && all == full);
    CHECK(located_list(s, 400, 4096, all) == 9 && all == full);
    CHECK(located_list(s, 400, 8, all) == 9 && (all == V{10, 60, 120, 180 | LAG, 260, 350, 420 | LAG, 480}));
    s.has_exit = false;  // the walk ended before the last chunk: nothing of `last` past own_hi
    CHECK(located_list(s, 400, 7, all) == 7 && (all == V{10, 60, 120, 180 | LAG, 210, 260, 350}));
}

int main()
{
    records();
    case_a_every_chunk_shares();
    case_b_no_shared_record();
    case_c_shared_record_after_first_owned();
    case_d_lag_bit_differs();
    case_e_walk_ends_early();
    case_f_frame_before_sample_0();
    case_g_record_overflow();
    case_h_located_list();
    if (g_failed) {
        fprintf(stderr, "stitch_selftest: %d checks failed\n", g_failed);
        return 1;
    }
    printf("stitch_selftest ok\n");
    return 0;
}
