// mac_selftest — the MAC kernels' per-lane steps and CRC arithmetic
// (csrc/ofdm_mac.hpp) on the CPU. The loops below are the kernels of
// ofdm_mac.hip with the 64 lanes of a wave as an array and the wave's
// reductions as loops; every load, store and table step is the shared code.
// The combine arithmetic is compared with a bytewise CRC-32 for every length
// 1..4200; whole frames are written and read back for every covered length
// 8..4200 and the GPU test's lengths, both chunk widths and both FCS kinds.
// The buffers are allocated to the byte, so that the sanitizers this is built
// with see any access outside them and any misaligned wide access. Host C++
// alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/ofdm_mac.hpp"

using namespace ofdm;

static const MacLanePow lane_pow = mac_make_lane_pow();
static MacTabs tabs;

static unsigned crc32_bytewise(const uint8_t* p, size_t n)
{
    unsigned c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int b = 0; b < 8; ++b) c = mac_bit_step(c);
    }
    return c ^ 0xffffffffu;
}

static void fill_tabs(unsigned krow)
{
    for (unsigned v = 0; v < 256; ++v) {
        mac_fill_t4(tabs, v);
        mac_fill_trow(tabs, v, krow);
    }
}

template <bool WIDE, bool CRC>
static void emu_write(const MacWriteArgs& a)
{
    constexpr unsigned W = WIDE ? 16 : 1;
    const unsigned rows = mac_rows(a.frame_len, W), nchunks = (a.frame_len + W - 1) / W;
    const unsigned fcs_c0 = a.m / W, fcs_c1 = (a.m + 3) / W;
    fill_tabs(a.k.krow);
    for (size_t f = 0; f < a.nframes; ++f) {
        const uint8_t* pl = a.payload + f * a.payload_stride;
        uint8_t* out = a.frames + f * a.frame_stride;
        const unsigned seq = a.seqs ? (unsigned)a.seqs[f] : (a.seq0 + (unsigned)f) & 0xffffu;
        const unsigned hdr_lo = a.tx_id | (a.rx_id << 16), hdr_hi = seq;
        unsigned sum = 0, crc = 0;
        for (unsigned lane = 0; lane < 64; ++lane) {
            unsigned lsum = 0, lcrc = 0;
            for (unsigned r = 0; r < rows; ++r) {
                const unsigned c = r * 64 + lane;
                unsigned wd[4] = {0u, 0u, 0u, 0u};
                if (c < nchunks) {
                    mac_build_chunk<WIDE>(pl, a.payload_len, hdr_lo, hdr_hi, c, wd);
                    const bool waits = c == 6 / W || c == 7 / W || (CRC && c >= fcs_c0 && c <= fcs_c1);
                    if (!waits) mac_store_chunk<WIDE>(out, c, wd, a.frame_stride);
                    lsum += mac_byte_sum(wd[0]) + mac_byte_sum(wd[1]) + mac_byte_sum(wd[2]) + mac_byte_sum(wd[3]);
                }
                if (CRC) {
                    if (r) lcrc = mac_lookup(tabs.trow, lcrc);
                    lcrc = mac_crc_chunk<WIDE>(tabs, lcrc, wd);
                }
            }
            sum += lsum;
            crc ^= mac_gf_mul(lcrc, lane_pow.p[WIDE ? 1 : 0][lane]);
        }
        const unsigned cs = sum & 0xffffu;
        if (CRC) crc = mac_gf_mul(crc, a.k.invz) ^ mac_gf_mul(mac_lookup(tabs.t4, cs << 16), a.k.csadv) ^ a.k.fin;
        for (unsigned lane = 0; lane < (CRC ? 6u : 2u); ++lane) {
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
        const unsigned zero[4] = {0u, 0u, 0u, 0u};
        for (size_t c = nchunks; c * W < a.frame_stride; ++c) mac_store_chunk<WIDE>(out, c, zero, a.frame_stride);
    }
}

struct Info {
    uint16_t tx_id, rx_id, seq_num, cs, cs_calc;
    uint8_t cs_ok, fcs_ok, ok, reserved[3];
};
static_assert(sizeof(Info) == 16, "ofdm_mac_info is 16 bytes");

template <bool WIDE, bool CRC>
static void emu_read(const MacReadArgs& a, unsigned* crc_out)
{
    constexpr unsigned W = WIDE ? 16 : 1;
    const unsigned rows = mac_rows(a.frame_len, W);
    fill_tabs(a.k.krow);
    for (size_t f = 0; f < a.nframes; ++f) {
        const uint8_t* in = a.frames + f * a.frame_stride;
        uint8_t* pl = a.payload ? a.payload + f * a.payload_stride : nullptr;
        unsigned sum = 0, crc = 0, hdr_lo = 0, hdr_hi = 0, fcs = 0;
        for (unsigned lane = 0; lane < 64; ++lane) {
            MacReadAcc acc{0u, 0u, 0u, 0u, 0u};
            for (unsigned r = 0; r < rows; ++r) {
                if (CRC && r) acc.crc = mac_lookup(tabs.trow, acc.crc);
                mac_read_chunk<WIDE, CRC>(tabs, in, pl, a.frame_len, a.m, r * 64 + lane, acc);
            }
            sum += acc.sum;
            hdr_lo ^= acc.hdr_lo;
            hdr_hi ^= acc.hdr_hi;
            fcs ^= acc.fcs;
            crc ^= mac_gf_mul(acc.crc, lane_pow.p[WIDE ? 1 : 0][lane]);
        }
        const unsigned cs_calc = sum & 0xffffu;
        unsigned fcs_ok = 1;
        if (CRC) {
            crc = mac_gf_mul(crc, a.k.invz) ^ a.k.fin;
            fcs_ok = crc == fcs;
            if (crc_out) crc_out[f] = crc;
        }
        const unsigned cs_ok = (hdr_hi >> 16) == cs_calc;
        const bool ok = cs_ok && fcs_ok && (a.expect_rx_id < 0 || (hdr_lo >> 16) == (unsigned)a.expect_rx_id);
        if (a.info) a.info[f] = MacU4{hdr_lo, hdr_hi, cs_calc | (cs_ok << 16) | (fcs_ok << 24), ok ? 1u : 0u};
        if (a.frame_errors && !ok) *a.frame_errors += 1;
    }
}

// The CRC-32 of n bytes by the wave's arithmetic alone: rows of 64 chunks, the
// row advance, the lanes' registers joined, the zero tail taken back, the
// initial value and the final inversion folded in. Any n from 1 (a frame has
// at least 8 covered bytes; the arithmetic does not care).
template <bool WIDE>
static unsigned wave_crc(const uint8_t* p, unsigned n)
{
    constexpr unsigned W = WIDE ? 16 : 1;
    const MacCrcK k = mac_crc_consts(n, 0, WIDE);
    const unsigned rows = mac_rows(n, W);
    fill_tabs(k.krow);
    unsigned crc = 0;
    for (unsigned lane = 0; lane < 64; ++lane) {
        unsigned reg = 0;
        for (unsigned r = 0; r < rows; ++r) {
            unsigned wd[4] = {0u, 0u, 0u, 0u};
            for (unsigned b = 0; b < W; ++b) {
                const unsigned o = (r * 64 + lane) * W + b;
                if (o < n) wd[b >> 2] |= (unsigned)p[o] << (8 * (b & 3u));
            }
            if (r) reg = mac_lookup(tabs.trow, reg);
            reg = mac_crc_chunk<WIDE>(tabs, reg, wd);
        }
        crc ^= mac_gf_mul(reg, lane_pow.p[WIDE ? 1 : 0][lane]);
    }
    return mac_gf_mul(crc, k.invz) ^ k.fin;
}

static unsigned rng_state = 12345;
static unsigned rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 24;
}

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (failures++ < 20) {            \
                std::printf("FAIL: ");        \
                std::printf(__VA_ARGS__);     \
                std::printf("\n");            \
            }                                 \
        }                                     \
    } while (0)

// A buffer of exactly n bytes that ends where its allocation ends and starts
// `mis` bytes past a 16-byte boundary.
struct Buf {
    uint8_t* base = nullptr;
    uint8_t* p;
    size_t n;
    Buf(size_t n_, unsigned mis) : n(n_)
    {
        if (posix_memalign(reinterpret_cast<void**>(&base), 16, n + mis + !(n + mis))) std::abort();
        p = base + mis;
        std::memset(base, 0xA5, n + mis);
    }
    ~Buf() { std::free(base); }
};

// nframes frames of one geometry: model frames bytewise, write them through
// the lane steps, read both back.
template <bool WIDE>
static void run_case(unsigned frame_len, bool crc, unsigned payload_len, size_t extra_stride, unsigned mis, size_t nframes)
{
    const unsigned F = crc ? 4 : 0, m = frame_len - F, cap = m - MAC_HDR;
    size_t fstride = frame_len + extra_stride, pstride = payload_len + extra_stride;
    if (WIDE) {  // what the wide path asks for: addresses and strides that are multiples of 4
        fstride = (fstride + 3) / 4 * 4;
        pstride = (pstride + 3) / 4 * 4;
        mis &= ~3u;
    }
    Buf pay((nframes - 1) * pstride + payload_len, WIDE ? (mis + 4) % 16 : mis);
    Buf frm(nframes * fstride, mis);
    for (size_t i = 0; i < pay.n; ++i) pay.p[i] = (uint8_t)rnd();
    std::vector<uint16_t> seqs(nframes);
    for (auto& s : seqs) s = (uint16_t)(rnd() | rnd() << 8);

    MacWriteArgs wa{};
    wa.payload = pay.p;
    wa.frames = frm.p;
    wa.seqs = seqs.data();
    wa.payload_stride = pstride;
    wa.frame_stride = fstride;
    wa.nframes = nframes;
    wa.payload_len = payload_len;
    wa.frame_len = frame_len;
    wa.m = m;
    wa.tx_id = 0xBEEF;
    wa.rx_id = 0x1234;
    wa.k = mac_crc_consts(frame_len, F, WIDE);
    if (crc) emu_write<WIDE, true>(wa);
    else emu_write<WIDE, false>(wa);

    std::vector<uint8_t> model(fstride);
    for (size_t f = 0; f < nframes; ++f) {
        std::fill(model.begin(), model.end(), 0);
        const uint16_t h[3] = {0xBEEF, 0x1234, seqs[f]};
        for (int i = 0; i < 3; ++i) {
            model[2 * i] = (uint8_t)(h[i] & 0xff);
            model[2 * i + 1] = (uint8_t)(h[i] >> 8);
        }
        std::memcpy(model.data() + 8, pay.p + f * pstride, payload_len);
        unsigned sum = 0;
        for (unsigned i = 0; i < m; ++i) sum += model[i];
        model[6] = (uint8_t)(sum & 0xff);
        model[7] = (uint8_t)((sum >> 8) & 0xff);
        if (crc) {
            const unsigned c = crc32_bytewise(model.data(), m);
            for (int i = 0; i < 4; ++i) model[m + i] = (uint8_t)(c >> (8 * i));
        }
        CHECK(!std::memcmp(model.data(), frm.p + f * fstride, fstride), "write W=%d len=%u crc=%d plen=%u frame %zu",
              WIDE ? 16 : 1, frame_len, (int)crc, payload_len, f);
    }

    // read back: exact-size input (the last frame ends at frame_len), guarded payload
    Buf in((nframes - 1) * fstride + frame_len, mis);
    std::memcpy(in.p, frm.p, in.n);
    if (nframes > 1) in.p[fstride + (cap ? 8 + (cap - 1) / 2 : 6)] ^= 0x10;  // frame 1 is damaged (cap 0: in its cs)
    size_t ostride = cap + extra_stride;
    if (WIDE) ostride = (ostride + 3) / 4 * 4;
    Buf outp((nframes - 1) * ostride + cap, WIDE ? (mis + 8) % 16 : mis);
    std::vector<MacU4> info(nframes);
    std::vector<unsigned> crcs(nframes, 0);
    unsigned long long errors = 0;
    MacReadArgs ra{};
    ra.frames = in.p;
    ra.payload = outp.p;
    ra.info = info.data();
    ra.frame_errors = &errors;
    ra.frame_stride = fstride;
    ra.payload_stride = ostride;
    ra.nframes = nframes;
    ra.frame_len = frame_len;
    ra.m = m;
    ra.expect_rx_id = 0x1234;
    ra.k = wa.k;
    if (crc) emu_read<WIDE, true>(ra, crcs.data());
    else emu_read<WIDE, false>(ra, nullptr);
    unsigned long long bad = 0;
    for (size_t f = 0; f < nframes; ++f) {
        Info i;
        std::memcpy(&i, &info[f], 16);
        const uint8_t* fr = in.p + f * fstride;
        unsigned sum = 0;
        for (unsigned k = 0; k < m; ++k)
            if (k != 6 && k != 7) sum += fr[k];
        const bool cs_ok = (uint16_t)sum == (uint16_t)(fr[6] | fr[7] << 8);
        bool fcs_ok = true;
        if (crc) {
            const unsigned c = crc32_bytewise(fr, m);
            CHECK(crcs[f] == c, "read crc W=%d len=%u frame %zu: %08x, bytewise %08x", WIDE ? 16 : 1, frame_len, f, crcs[f], c);
            unsigned got = 0;
            for (int k = 0; k < 4; ++k) got |= (unsigned)fr[m + k] << (8 * k);
            fcs_ok = got == c;
        }
        CHECK(i.tx_id == (fr[0] | fr[1] << 8) && i.rx_id == (fr[2] | fr[3] << 8) && i.seq_num == (fr[4] | fr[5] << 8) &&
                  i.cs == (fr[6] | fr[7] << 8) && i.cs_calc == (uint16_t)sum && i.cs_ok == cs_ok && i.fcs_ok == fcs_ok &&
                  i.ok == (cs_ok && fcs_ok) && !i.reserved[0] && !i.reserved[1] && !i.reserved[2],
              "read info W=%d len=%u crc=%d frame %zu", WIDE ? 16 : 1, frame_len, (int)crc, f);
        if (f == 1) CHECK(!i.ok, "damaged frame passes: len=%u crc=%d", frame_len, (int)crc);
        else CHECK(i.ok, "good frame fails: W=%d len=%u crc=%d frame %zu", WIDE ? 16 : 1, frame_len, (int)crc, f);
        bad += !i.ok;
        CHECK(!std::memcmp(outp.p + f * ostride, fr + 8, cap), "read payload W=%d len=%u frame %zu", WIDE ? 16 : 1, frame_len, f);
        if (f + 1 < nframes)
            for (size_t k = cap; k < ostride; ++k) CHECK(outp.p[f * ostride + k] == 0xA5, "payload guard len=%u", frame_len);
    }
    CHECK(errors == bad, "frame_errors %llu, expected %llu", errors, bad);
}

int main()
{
    // the arithmetic itself
    CHECK(mac_gf_mul(mac_xpow(8 * 5), mac_xpow(MAC_ORDER - 8 * 5)) == 0x80000000u, "x^40 x^-40 != 1");
    CHECK(mac_xpow(MAC_ORDER) == 0x80000000u, "x^(2^32-1) != 1");
    const uint8_t check[9] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
    CHECK(crc32_bytewise(check, 9) == 0xCBF43926u, "bytewise CRC-32 check value");

    // the combine arithmetic on every length 1..4200, both chunk widths
    {
        std::vector<uint8_t> msg(4200);
        for (auto& b : msg) b = (uint8_t)rnd();
        for (unsigned n = 1; n <= 4200; ++n) {
            const unsigned want = crc32_bytewise(msg.data(), n);
            const unsigned w16 = wave_crc<true>(msg.data(), n), w1 = wave_crc<false>(msg.data(), n);
            CHECK(w16 == want && w1 == want, "combine n=%u: wide %08x, narrow %08x, bytewise %08x", n, w16, w1, want);
        }
    }
    // and through the kernels' own steps, as frames: every covered length 8..4200
    for (unsigned m = 8; m <= 4200; ++m) {
        const unsigned cap = m - 8;
        run_case<true>(m + 4, true, cap, 0, m % 16, 2);
        run_case<false>(m + 4, true, cap, m % 4, m % 16, 2);
    }
    // both FCS kinds, partial payloads, strides past the length, every misalignment
    const unsigned lens[] = {8, 9, 12, 13, 15, 16, 17, 63, 64, 65, 255, 1023, 1024, 1025, 4096, 4099, 65536};
    for (unsigned len : lens)
        for (int crc = 0; crc < 2; ++crc) {
            if (len < 8u + 4u * crc) continue;
            const unsigned cap = len - 8 - 4 * crc;
            const unsigned pls[4] = {0, 1, cap ? cap - 1 : 0, cap};
            for (unsigned pl : pls) {
                if (pl > cap) continue;
                for (unsigned mis : {0u, 4u, 12u}) {
                    run_case<true>(len, crc, pl, 0, mis, 5);
                    run_case<true>(len, crc, pl, 3, mis, 3);
                }
                for (unsigned mis : {0u, 1u, 7u, 15u}) {
                    run_case<false>(len, crc, pl, 0, mis, 5);
                    run_case<false>(len, crc, pl, 3, mis, 3);
                }
            }
        }
    if (failures) {
        std::printf("mac_selftest: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("mac_selftest: ok\n");
    return 0;
}
