// ofdm_mac.hpp — the MAC framing of include/ofdm_mi355x.h ("MAC framing and
// frame check"): the CRC-32 arithmetic, the per-launch constants and the
// per-lane steps of the kernels of ofdm_mac.hip. Plain C++: the host builds the
// constants from it, and apps/mac_selftest.cpp runs the same per-lane steps on
// the CPU, lane by lane, against a bytewise CRC (DESIGN.md "MAC framing").
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define OFDM_MAC_HD __host__ __device__
#else
#define OFDM_MAC_HD
#endif

namespace ofdm {

constexpr unsigned MAC_POLY = 0xEDB88320u;   // CRC-32/IEEE 802.3, reflected
constexpr unsigned MAC_HDR = 8;              // tx_id, rx_id, seq_num, cs
constexpr unsigned MAC_MAX_FRAME = 65536;
constexpr int MAC_THREADS = 256;
constexpr int MAC_WAVES = MAC_THREADS / 64;  // one wave per frame at a time
constexpr long MAC_MAX_GRID = 2048;          // workgroups; the waves stride over the frames beyond

// GF(2)[x] mod P on reflected 32-bit values (bit 31 is x^0): a CRC register
// that runs over n zero bytes is multiplied by x^(8n).
OFDM_MAC_HD constexpr unsigned mac_gf_mul(unsigned a, unsigned b)
{
    unsigned p = 0;
    // (kept a loop on the device: unrolled, the 32 masks of every constant
    // factor are hoisted out of the frame loop and take 32 registers each)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (MAC_POLY & (0u - (b & 1u)));
    }
    return p;
}

// x^e mod P. P is primitive: x^(2^32 - 1) = 1, which gives the negative powers.
constexpr unsigned long long MAC_ORDER = 0xffffffffull;
constexpr unsigned mac_xpow(unsigned long long e)
{
    unsigned r = 0x80000000u, p = 0x40000000u;
    for (; e; e >>= 1) {
        if (e & 1) r = mac_gf_mul(r, p);
        p = mac_gf_mul(p, p);
    }
    return r;
}

// One bit step of the register over a zero bit.
OFDM_MAC_HD constexpr unsigned mac_bit_step(unsigned c) { return (c >> 1) ^ (MAC_POLY & (0u - (c & 1u))); }

// The tables a workgroup keeps in LDS: t4[s][v] is the register v << 8s run
// over 4 zero bytes (the slice-by-4 tables), trow[s][v] the same register
// times krow (below).
struct MacTabs {
    unsigned t4[4][256];
    unsigned trow[4][256];
};

// Entry v of the four t4 tables: v << 8s after 32 bit steps is v after 32 - 8s.
OFDM_MAC_HD inline void mac_fill_t4(MacTabs& t, unsigned v)
{
    unsigned c = v;
    for (int s = 3; s >= 0; --s) {
        for (int i = 0; i < 8; ++i) c = mac_bit_step(c);
        t.t4[s][v] = c;
    }
}
OFDM_MAC_HD inline void mac_fill_trow(MacTabs& t, unsigned v, unsigned krow)
{
    for (int s = 0; s < 4; ++s) t.trow[s][v] = mac_gf_mul(v << (8 * s), krow);
}
OFDM_MAC_HD inline unsigned mac_lookup(const unsigned (*t)[256], unsigned c)
{
    return t[0][c & 0xffu] ^ t[1][(c >> 8) & 0xffu] ^ t[2][(c >> 16) & 0xffu] ^ t[3][c >> 24];
}

// The tiling. A lane holds a chunk of W bytes of the frame (16: four
// little-endian words, or 1), the wave a row of 64 chunks, and a frame has
// `rows` rows. The sum and the CRC cover bytes [0, m), m = frame_len - F; the
// bytes of the rows past m count as zeros, z of them.
OFDM_MAC_HD constexpr unsigned mac_rows(unsigned frame_len, unsigned w) { return (frame_len + 64 * w - 1) / (64 * w); }

// The CRC constants of a launch (every frame of it has the same lengths). With
// raw(A) the register after message A from a zero start, raw(A ++ B) =
// raw(A) x^(8|B|) ^ raw(B), and a lane's words go through the register four
// bytes at a time, so that before a row's words the lane's register advances
// by the rest of the row (krow). The lanes' registers are joined as
// sum_l reg_l x^(8W(63-l)) (mac_lane_pow), the z zero bytes are taken back
// (invz), the initial 0xffffffff run over m bytes and the final inversion are
// one constant (fin), and the frame writer adds the checksum's two bytes, which
// it knows last, as raw(0, 0, cs_lo, cs_hi) x^(8(m-8)) (csadv).
struct MacCrcK {
    unsigned krow, invz, fin, csadv;
};

inline MacCrcK mac_crc_consts(unsigned frame_len, unsigned fcs_bytes, bool wide)
{
    const unsigned w = wide ? 16 : 1, m = frame_len - fcs_bytes;
    const unsigned long long z = (unsigned long long)mac_rows(frame_len, w) * 64 * w - m;
    MacCrcK k{};
    k.krow = mac_xpow(8ull * (64 * w - (wide ? 16 : 4)));
    k.invz = mac_xpow(MAC_ORDER - (8ull * z) % MAC_ORDER);
    k.fin = mac_gf_mul(0xffffffffu, mac_xpow(8ull * m)) ^ 0xffffffffu;
    k.csadv = mac_xpow(8ull * (m - MAC_HDR));
    return k;
}

// x^(8W(63-l)) for lane l; [0]: W = 1, [1]: W = 16.
struct MacLanePow {
    unsigned p[2][64];
};
constexpr MacLanePow mac_make_lane_pow()
{
    MacLanePow t{};
    for (int wi = 0; wi < 2; ++wi) {
        const unsigned step = mac_xpow(wi ? 128 : 8);
        unsigned v = 0x80000000u;
        for (int l = 63; l >= 0; --l) {
            t.p[wi][l] = v;
            v = mac_gf_mul(v, step);
        }
    }
    return t;
}

// 16 bytes of a buffer: a wide access needs its address 4-byte aligned only.
struct alignas(4) MacU4 {
    unsigned x, y, z, w;
};

struct MacWriteArgs {
    const uint8_t* payload;
    uint8_t* frames;
    const uint16_t* seqs;             // nullable
    size_t payload_stride, frame_stride, nframes;
    unsigned payload_len, frame_len, m;   // m = frame_len - F
    unsigned tx_id, rx_id, seq0;
    MacCrcK k;
};

struct MacReadArgs {
    const uint8_t* frames;
    uint8_t* payload;                 // nullable
    MacU4* info;                      // nullable: one ofdm_mac_info per frame
    unsigned long long* frame_errors; // nullable
    size_t frame_stride, payload_stride, nframes;
    unsigned frame_len, m;
    int expect_rx_id;
    MacCrcK k;
};

// The register over a chunk's words; a single byte is the last of four, behind
// three zero bytes, which leave a register as it is.
template <bool WIDE>
OFDM_MAC_HD inline unsigned mac_crc_chunk(const MacTabs& t, unsigned c, const unsigned wd[4])
{
    if (WIDE) {
        for (int i = 0; i < 4; ++i) c = mac_lookup(t.t4, c ^ wd[i]);
        return c;
    }
    return mac_lookup(t.t4, c ^ (wd[0] << 24));
}

OFDM_MAC_HD inline unsigned mac_byte_sum(unsigned w)
{
    return (w & 0xffu) + ((w >> 8) & 0xffu) + ((w >> 16) & 0xffu) + (w >> 24);
}

// Puts the nb low bytes of v at frame offsets off .. off + nb - 1, where they
// fall into chunk c.
template <bool WIDE>
OFDM_MAC_HD inline void mac_place(unsigned wd[4], unsigned c, unsigned off, unsigned v, int nb)
{
    constexpr unsigned W = WIDE ? 16 : 1;
    for (int b = 0; b < nb; ++b) {
        const unsigned o = off + (unsigned)b;
        if (o / W != c) continue;
        const unsigned byte = (v >> (8 * b)) & 0xffu, pos = o % W;
        for (unsigned i = 0; i < 4; ++i)
            if (i == pos >> 2) wd[i] |= byte << (8 * (pos & 3u));
    }
}

// The payload word at offset p (4-byte aligned), zeros from plen on.
OFDM_MAC_HD inline unsigned mac_payload_word(const uint8_t* pl, unsigned plen, unsigned p)
{
    if (p + 4 <= plen) return *reinterpret_cast<const unsigned*>(pl + p);
    unsigned v = 0;
    for (unsigned b = 0; b < 4; ++b)
        if (p + b < plen) v |= (unsigned)pl[p + b] << (8 * b);
    return v;
}

// Chunk c (inside the frame) of the frame to write, its cs and FCS bytes 0.
template <bool WIDE>
OFDM_MAC_HD inline void mac_build_chunk(const uint8_t* pl, unsigned plen, unsigned hdr_lo, unsigned hdr_hi, unsigned c,
                                        unsigned wd[4])
{
    if (WIDE) {
        if (c >= 1 && 16 * c + 8 <= plen) {
            const MacU4 v = *reinterpret_cast<const MacU4*>(pl + (16 * c - 8));
            wd[0] = v.x;
            wd[1] = v.y;
            wd[2] = v.z;
            wd[3] = v.w;
            return;
        }
        wd[0] = c ? mac_payload_word(pl, plen, 16 * c - 8) : hdr_lo;
        wd[1] = c ? mac_payload_word(pl, plen, 16 * c - 4) : hdr_hi;
        wd[2] = mac_payload_word(pl, plen, 16 * c);
        wd[3] = mac_payload_word(pl, plen, 16 * c + 4);
    } else {
        wd[0] = c < 8 ? ((c < 4 ? hdr_lo : hdr_hi) >> (8 * (c & 3u))) & 0xffu : c - 8 < plen ? pl[c - 8] : 0u;
        wd[1] = wd[2] = wd[3] = 0;
    }
}

// Stores chunk c of a frame whose frame_stride bytes end at `limit` (a
// multiple of 4 where WIDE): the last chunk may be cut there.
template <bool WIDE>
OFDM_MAC_HD inline void mac_store_chunk(uint8_t* out, size_t c, const unsigned wd[4], size_t limit)
{
    if (WIDE) {
        if (16 * c + 16 <= limit) {
            *reinterpret_cast<MacU4*>(out + 16 * c) = MacU4{wd[0], wd[1], wd[2], wd[3]};
        } else {
            for (unsigned i = 0; i < 4; ++i)
                if (16 * c + 4 * i + 4 <= limit) *reinterpret_cast<unsigned*>(out + 16 * c + 4 * i) = wd[i];
        }
    } else {
        out[c] = (uint8_t)wd[0];
    }
}

// What a lane gathers over the rows of a received frame.
struct MacReadAcc {
    unsigned sum, crc, hdr_lo, hdr_hi, fcs;
};

// Chunk c of a received frame: loads it (no byte at or past frame_len is
// read), adds its bytes below m to the sum (without 6 and 7) and to the
// register, copies those from 8 on to the payload, and keeps the header's and
// the FCS's bytes.
template <bool WIDE, bool CRC>
OFDM_MAC_HD inline void mac_read_chunk(const MacTabs& t, const uint8_t* in, uint8_t* pl, unsigned frame_len, unsigned m,
                                       unsigned c, MacReadAcc& r)
{
    constexpr unsigned W = WIDE ? 16 : 1;
    const unsigned o0 = c * W;
    unsigned wd[4] = {0u, 0u, 0u, 0u};
    if (WIDE && c >= 1 && o0 + 16 <= m) {
        const MacU4 v = *reinterpret_cast<const MacU4*>(in + o0);
        wd[0] = v.x;
        wd[1] = v.y;
        wd[2] = v.z;
        wd[3] = v.w;
        r.sum += mac_byte_sum(v.x) + mac_byte_sum(v.y) + mac_byte_sum(v.z) + mac_byte_sum(v.w);
        if (pl) *reinterpret_cast<MacU4*>(pl + (o0 - 8)) = v;
    } else {
        for (unsigned b = 0; b < W; ++b) {
            const unsigned o = o0 + b;
            if (o >= frame_len) break;
            const unsigned v = in[o];
            if (o < 8) {
                if (o < 4) r.hdr_lo |= v << (8 * o);
                else r.hdr_hi |= v << (8 * (o - 4));
            }
            if (o < m) {
                if (o != 6 && o != 7) r.sum += v;
                for (unsigned i = 0; i < 4; ++i)
                    if (i == b >> 2) wd[i] |= v << (8 * (b & 3u));
                if (o >= 8 && pl) pl[o - 8] = (uint8_t)v;
            } else if (CRC) {
                r.fcs |= v << (8 * (o - m));
            }
        }
    }
    if (CRC) r.crc = mac_crc_chunk<WIDE>(t, r.crc, wd);
}

#if defined(__HIPCC__)
// Launchers (ofdm_mac.hip): `crc` selects OFDM_FCS_CRC32; a.k is filled in by them.
hipError_t launch_mac_write(MacWriteArgs a, bool crc, hipStream_t stream);
hipError_t launch_mac_read(MacReadArgs a, bool crc, hipStream_t stream);
#endif

}  // namespace ofdm
