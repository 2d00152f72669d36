// tables_selftest — every table of csrc/ofdm_tables.hpp (what ofdm_create and
// cfo_plan upload) computed on the CPU and written out for
// tests/test_tables_selftest.py to compare with the oracle. Host C++ alone,
// built with the host sanitizers.
//
//   tables_selftest <the 19 ofdm_params fields, in order> <out dir> <preamble file> [nsym ...]
//
// Each table goes to <out dir>/<name>.<type> as a raw little-endian array
// (i32, u32, i64, u8; f64 with complex values as re, im pairs). The preamble
// file holds the OFDM preamble as complex doubles: the template and its
// spectrum are made from it. Each nsym adds cfo_<nsym>.i32 = {g, logm, the
// P + 2 borders} (g = 0, logm = -1: no kernel covers the form length). Exit
// status 1 with the error's text when the layout does not fit.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../csrc/ofdm_sync.hpp"
#include "../csrc/ofdm_tables.hpp"

namespace T = ofdm::tables;

static std::string g_dir;

template <class V>
static void dump(const char* name, const std::vector<V>& v)
{
    const std::string path = g_dir + "/" + name;
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || (!v.empty() && fwrite(v.data(), sizeof(V), v.size(), f) != v.size()) || fclose(f)) {
        fprintf(stderr, "tables_selftest: cannot write %s\n", path.c_str());
        exit(2);
    }
}

static int usage(const char* why)
{
    fprintf(stderr, "tables_selftest: %s\n", why);
    return 2;
}

int main(int argc, char** argv)
{
    if (argc < 22) return usage("need 19 parameters, an output directory and a preamble file");
    long v[19];
    for (int i = 0; i < 19; ++i) v[i] = atol(argv[1 + i]);
    const ofdm_params p{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9],
                        v[10], v[11], v[12], v[13], v[14], v[15], v[16], v[17], v[18]};
    g_dir = argv[20];
    const long N = p.fft_size, D = p.num_data_subc, P = p.num_pilot_subc;
    if (T::ilog2_exact(N) < 6 || T::ilog2_exact(N) > 12 || P < 1 || P > 256 || D < P || D % P)
        return usage("fft_size / num_data_subc / num_pilot_subc outside what ofdm_create accepts");
    if (p.t2sin_size < 0 || p.t2sin_size > (1 << 20) ||
        (p.t2sin_size && (p.t2_sin_f1 < 0 || p.t2_sin_f1 >= p.t2sin_size || p.t2_sin_f2 < 0 || p.t2_sin_f2 >= p.t2sin_size)))
        return usage("T2 tones outside T2sin_size");

    T::Layout lay;
    if (const char* why = T::carrier_layout(N, D, P, lay)) {
        printf("%s\n", why);
        return 1;
    }
    const ofdm_geometry g = T::geometry(p);
    dump("geometry.i64", std::vector<long>{g.symbol_len, g.message_len, g.preamble_len, g.frame_len, g.ring_len,
                                           g.data_per_frame, g.bytes_per_frame, g.segment_size});
    dump("pilot.i32", lay.pilot);
    dump("segst.i32", lay.segst);
    dump("data_bin.i32", lay.data_bin);
    dump("data_slot.i32", lay.data_slot);
    dump("bin_map.i32", lay.bin_map);
    dump("rx_pack.i32", T::rx_pack(lay, (int)N));
    dump("pilot_swz.i32", T::pilot_swz(lay, (int)N));
    const std::vector<int> tx_code = T::tx_code(lay);
    dump("tx_code.i32", tx_code);
    dump("tx_dead.u32", ofdm::tx_dead_masks(tx_code));
    for (int k : {1, 2, 4, 6, 8}) dump(("constellation_" + std::to_string(k) + ".f64").c_str(), T::constellation(k));
    dump("t2_symbol.f64", T::t2_symbol((int)p.t2sin_size, p.t2_sin_f1, p.t2_sin_f2));
    dump("t2_mask.f64", T::t2_mask((int)p.t2sin_size, (int)p.t2_sin_f1, (int)p.t2_sin_f2, (int)p.smooth));
    const std::vector<uint8_t> bytes = T::preamble_bytes(D * p.num_pr_symb / 8, p.pr_seed);
    dump("preamble_bytes.u8", bytes);
    dump("mod_preamble.f64", T::mod_preamble(bytes, (long)bytes.size() * 8));

    std::vector<T::cd> pre(g.preamble_len);
    FILE* f = fopen(argv[21], "rb");
    if (!f || fread(pre.data(), sizeof(T::cd), pre.size(), f) != pre.size()) return usage("cannot read the preamble file");
    fclose(f);
    if (p.pr_sin_len < 0 || p.pr_sin_len > g.preamble_len) return usage("pr_sin_len exceeds the preamble");
    const std::vector<T::cd> templ = T::preamble_template(pre, (int)p.pr_sin_len);
    dump("templ.f64", templ);
    if (p.pr_sin_len <= ofdm::WALK_FFT_M - 63) {  // as ofdm_create: the walker's FFT search covers it
        double tmax = 0.0;
        dump("tspec.f64", T::template_spectrum(templ, ofdm::WALK_FFT_M, &tmax));
        dump("tspec_max.f64", std::vector<double>{tmax});
    }
    for (int i = 22; i < argc; ++i) {
        const long nsym = atol(argv[i]), S = g.symbol_len * nsym;
        std::vector<int> out{0, -1};
        (void)T::cfo_shape(S, &out[0], &out[1]);
        const std::vector<int> b = T::cfo_borders((int)N, (int)D, (int)P, S);
        out.insert(out.end(), b.begin(), b.end());
        dump(("cfo_" + std::to_string(nsym) + ".i32").c_str(), out);
    }
    printf("tables_selftest: ok\n");
    return 0;
}
