// ofdm_tables.hpp — the constants of a modem context as plain host arithmetic:
// numbers and vectors in, vectors out. No HIP runtime call and no context, so
// apps/tables_selftest.cpp checks every one of them on the CPU
// (tests/test_tables_selftest.py); ofdm_create.cpp uploads what they return.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <random>
#include <vector>

#include "../../include/ofdm_mi355x.h"
#include "ofdm_internal.hpp"

namespace ofdm::tables {

using cd = std::complex<double>;

inline int ilog2_exact(long n)
{
    if (n <= 0 || (n & (n - 1))) return -1;
    int l = 0;
    while ((1L << l) < n) ++l;
    return l;
}

// FRAME_FORM ctor (Frame.cpp:213-232); the pilot and segment bins are the layout's
inline ofdm_geometry geometry(const ofdm_params& p)
{
    const int L = (int)p.fft_size + (int)p.cp_size, D = (int)p.num_data_subc, S = (int)p.num_symb;
    const int npr = (int)p.num_pr_symb, t2 = (int)p.t2sin_size, k = (int)p.mod_type;
    ofdm_geometry g{};
    g.symbol_len = L;
    g.message_len = (long)L * S;
    g.preamble_len = (long)L * npr;
    g.frame_len = t2 + g.preamble_len + g.message_len;
    g.ring_len = g.frame_len * (p.rx_buf_size + 1);
    g.data_per_frame = (long)D * S;
    g.bytes_per_frame = (long)D * S * k / 8;
    g.segment_size = D / (int)p.num_pilot_subc;
    return g;
}

// FFT_FORM layout (Frame.cpp:31-44): P pilots in two combs around the unused
// middle, each with its segment of D/P data bins (below the pilot in the lower
// comb, above it in the upper). bin_map: >= 0 data index, -1 unused, -2 pilot.
struct Layout {
    std::vector<int> pilot, segst, data_bin, data_slot, bin_map;
};

// Needs N > 0 and 1 <= P <= D, D a multiple of P. Returns null, or why the
// layout does not stay inside [1, N) without collisions.
inline const char* carrier_layout(long N, long D, long P, Layout& o)
{
    const long step = D / P + 1, seg = D / P, half = P / 2;
    o = Layout{};
    o.pilot.assign(P, 0);
    o.segst.assign(P, 0);
    o.bin_map.assign(N, -1);
    long j = 0;
    auto take = [&](long b, long what) {
        if (b < 1 || b >= N || o.bin_map[b] != -1) return false;
        o.bin_map[b] = (int)what;
        return true;
    };
    auto slot = [&](long pilot, long first) -> const char* {  // pilot j and its segment
        if (!take(pilot, -2)) return "pilot comb does not fit fft_size";
        o.pilot[j] = (int)pilot;
        o.segst[j] = (int)first;
        for (long t = 0; t < seg; ++t) {
            if (!take(first + t, j * seg + t)) return "data segments do not fit fft_size";
            o.data_bin.push_back((int)(first + t));
            o.data_slot.push_back((int)j);
        }
        return nullptr;
    };
    const char* why = nullptr;
    for (long pos = 1 + seg; j < half && !why; ++j, pos += step) why = slot(pos, pos - seg);
    for (long pos = N - step * half; j < P && !why; ++j, pos += step) why = slot(pos, pos + 1);
    return why;
}

// rx per-thread tables, zero-padded to the rx kernel's fixed per-thread
// counts (RX_DPT data and one pilot per thread) so it loads them unguarded
inline std::vector<int> rx_pack(const Layout& l, int N)
{
    const int D = (int)l.data_bin.size();
    std::vector<int> t(std::max(D, RX_DPT * (N / 8)), 0);
    for (int d = 0; d < D; ++d) t[d] = lds_swz_host(l.data_bin[d]) | (l.data_slot[d] << 16);
    return t;
}

inline std::vector<int> pilot_swz(const Layout& l, int N)
{
    const int P = (int)l.pilot.size();
    std::vector<int> t(std::max(P, N / 8), 0);
    for (int j = 0; j < P; ++j) t[j] = lds_swz_host(l.pilot[j]);
    return t;
}

// tx per-bin codes (ofdm_internal.hpp tx_code): data index + 0xff mask, or
// the pilot / zero entry of the kernel's LDS point table. The dead-group masks
// are tx_dead_masks of this table.
inline std::vector<int> tx_code(const Layout& l)
{
    std::vector<int> t(l.bin_map.size());
    for (size_t b = 0; b < t.size(); ++b)
        t[b] = l.bin_map[b] >= 0 ? tx_code_data(l.bin_map[b])
                                 : tx_code_fixed(l.bin_map[b] == -2 ? TX_LDS_PILOT : TX_LDS_ZERO);
    return t;
}

// Modulation::Modulation table (modulation.cpp:4-36).
inline std::vector<double2> constellation(int k)
{
    std::vector<double2> t(1u << k);
    if (k == 1) {
        const double step = M_PI * 2 / (double)2;
        for (int i = 0; i < 2; ++i) {
            const cd z = std::exp(cd(0.0, 1.0) * (step * cd(i) + M_PI_4 * 5));
            t[i] = make_double2(z.real(), z.imag());
        }
    } else {
        const unsigned num = 1u << (k / 2);
        for (unsigned i = 0; i < t.size(); ++i) {
            const uint8_t in = (uint8_t)i;
            t[i] = make_double2(2.0 / (num - 1) * double(in % num) - 1.0, 2.0 / (num - 1) * double(in >> (k / 2)) - 1.0);
        }
    }
    return t;
}

// T2SIN_FORM::set (Frame.cpp:139-154): X[f1] = X[f2] = 0.5, unnormalised
// backward DFT of T2sin_size points = two complex tones of amplitude 0.5.
inline std::vector<cd> t2_symbol(int t2, long f1, long f2)
{
    std::vector<cd> sym(t2, cd(0, 0));
    if (t2) {
        std::vector<cd> spec(t2, cd(0, 0));
        spec[f1] = cd(0.5, 0);
        spec[f2] = cd(0.5, 0);
        for (int n = 0; n < t2; ++n) {
            cd acc(0, 0);
            for (int kk = 0; kk < t2; ++kk) {
                if (spec[kk] == cd(0, 0)) continue;
                const double a = 2.0 * M_PI * (double)(((long)kk * n) % t2) / (double)t2;
                acc += spec[kk] * cd(std::cos(a), std::sin(a));
            }
            sym[n] = acc;
        }
    }
    return sym;
}

// T2 detector mask (Frame.cpp:120-133)
inline std::vector<double> t2_mask(int t2, int f1, int f2, int sm)
{
    std::vector<double> mask(std::max(1, t2), 0.0);
    if (t2) {
        for (int i = std::max(0, f1 - sm); i <= std::min(t2 - 1, f1 + sm); ++i) mask[i] += 1.0;
        for (int i = std::max(0, f2 - sm); i <= std::min(t2 - 1, f2 + sm); ++i) mask[i] += 1.0;
    }
    return mask;
}

// PREAMBLE_FORM (Frame.cpp:259-294): mt19937(pr_seed) bytes
inline std::vector<uint8_t> preamble_bytes(long nb, long seed)
{
    std::vector<uint8_t> bytes(nb);
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> dist(0, 255);
    for (auto& b : bytes) b = (uint8_t)dist(rng);
    return bytes;
}

// mod_preamble = Mod.mod(preamble) (BPSK points, bit_stream_converter(1,8))
inline std::vector<cd> mod_preamble(const std::vector<uint8_t>& bytes, long npoints)
{
    const auto bp = constellation(1);
    std::vector<cd> mp(npoints);
    for (long i = 0; i < npoints; ++i) {
        const int bit = (bytes[i >> 3] >> (7 - (i & 7))) & 1;
        mp[i] = cd(bp[bit].x, bp[bit].y);
    }
    return mp;
}

// the detector's template: the conjugate of the preamble's first Lt samples, normalised
inline std::vector<cd> preamble_template(const std::vector<cd>& ofdm_preamble, int Lt)
{
    std::vector<cd> templ(Lt);
    double norm = 0.0;
    for (int i = 0; i < Lt; ++i) {
        templ[i] = std::conj(ofdm_preamble[i]);
        norm += std::abs(templ[i] * templ[i]);
    }
    norm = std::sqrt(norm);
    for (int i = 0; i < Lt; ++i) templ[i] /= cd(norm);
    return templ;
}

// stream walker FFT search (ofdm_sync.hip walk_preamble_fft): template
// spectrum tspec_k = sum_j c_j e^{+2 pi i k j / M}, long double; *max_abs: the
// largest magnitude of the rounded spectrum
inline std::vector<double2> template_spectrum(const std::vector<cd>& templ, int M, double* max_abs)
{
    std::vector<double2> tsp(M);
    *max_abs = 0.0;
    for (int k = 0; k < M; ++k) {
        long double re = 0, im = 0;
        for (size_t j = 0; j < templ.size(); ++j) {
            const long double a = 2.0L * 3.14159265358979323846264338327950288L * (long double)((k * (long)j) % M) / M;
            const long double cr = templ[j].real(), ci = templ[j].imag();
            const long double co = cosl(a), si = sinl(a);
            re += cr * co - ci * si;
            im += cr * si + ci * co;
        }
        tsp[k] = make_double2((double)re, (double)im);
        *max_abs = std::max(*max_abs, std::hypot(tsp[k].x, tsp[k].y));
    }
    return tsp;
}

// pilot_freq_sinh on a form of S samples: S = M (g = 1, M = 2^logm up to 4096)
// or 5 M (g = 5, M up to 1024), M >= 64; false: no kernel covers the length
inline bool cfo_shape(long S, int* g, int* logm)
{
    if (ilog2_exact(S) >= 6 && ilog2_exact(S) <= 12) {
        *g = 1;
        *logm = ilog2_exact(S);
    } else if (S % 5 == 0 && ilog2_exact(S / 5) >= 6 && ilog2_exact(S / 5) <= 10) {
        *g = 5;
        *logm = ilog2_exact(S / 5);
    } else {
        return false;
    }
    return true;
}

// its P + 2 window borders, exactly as Frame.hpp:311-321 computes them
inline std::vector<int> cfo_borders(int N, int D, int P, long S)
{
    const double rel_bw = double(D + P) / (N);
    const double rel_pilot_w = rel_bw / P;
    const int pilot_w = int(S * rel_pilot_w);
    std::vector<int> borders(P + 2);
    for (int i = 0, j = int((1.0 - rel_bw - rel_pilot_w) / 2.0 * S); i < P + 2; i++) {
        borders[i] = j;
        j += pilot_w;
    }
    borders[0] = std::max(0, borders[0]);
    return borders;
}

}  // namespace ofdm::tables
