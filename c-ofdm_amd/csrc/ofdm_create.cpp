// ofdm_create.cpp — the life cycle of a modem context: parameter defaults and
// config parsing, validation, ofdm_create as a chain of named steps (the
// arithmetic of every table is in ofdm_tables.hpp; the steps upload what it
// returns), ofdm_destroy, and the CFO plans that later calls add. What a step
// allocates is held by an owner (ofdm_owned.hpp) from the moment it exists, so
// a step that fails leaves nothing behind.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <climits>
#include <cmath>
#include <fstream>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "ofdm_ctx.hpp"
#include "ofdm_sync.hpp"
#include "ofdm_tables.hpp"

namespace tables = ofdm::tables;
using ofdm::DevBuf;
using ofdm::fail;
using ofdm::hip_fail;
using ofdm::twiddles;  // ofdm_internal.hpp
using tables::ilog2_exact;

namespace {

// key=value ConfigMap exactly as parse_config (config/parser.cpp:4-33):
// trim, skip blank and '#' lines and lines without '=', strip every space
// from key and value, std::stol the value (throws -> OFDM_ERR_PARSE).
int parse_file(const char* path, std::unordered_map<std::string, long>& cfg)
{
    if (!path) return fail(OFDM_ERR_INVALID, "null config path");
    std::ifstream file(path);
    if (!file.is_open()) return fail(OFDM_ERR_IO, "Cannot open config file");
    std::string line;
    while (std::getline(file, line)) {
        line.erase(line.begin(), std::find_if(line.begin(), line.end(),
                                              [](unsigned char ch) { return !std::isspace(ch); }));
        line.erase(std::find_if(line.rbegin(), line.rend(), [](unsigned char ch) { return !std::isspace(ch); })
                       .base(),
                   line.end());
        if (line.empty() || line[0] == '#') continue;
        auto pos = line.find('=');
        if (pos == std::string::npos) continue;
        std::string key = line.substr(0, pos), value = line.substr(pos + 1);
        key.erase(std::remove_if(key.begin(), key.end(), ::isspace), key.end());
        value.erase(std::remove_if(value.begin(), value.end(), ::isspace), value.end());
        try {
            cfg[key] = std::stol(value);
        } catch (const std::exception& e) {
            return fail(OFDM_ERR_PARSE, "stol failed for key '%s': %s", key.c_str(), e.what());
        }
    }
    return OFDM_OK;
}

template <class T>
int upload(DevBuf<T>& dst, const std::vector<T>& v)
{
    HIP_TRY(hipMalloc((void**)dst.put(), std::max<size_t>(1, v.size()) * sizeof(T)));
    if (!v.empty()) HIP_TRY(hipMemcpy(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return OFDM_OK;
}

std::vector<double2> as_double2(const std::vector<cd>& v)
{
    std::vector<double2> o(v.size());
    for (size_t i = 0; i < v.size(); ++i) o[i] = make_double2(v[i].real(), v[i].imag());
    return o;
}

int validate(const ofdm_params* p)
{
    const long N = p->fft_size, D = p->num_data_subc, P = p->num_pilot_subc, k = p->mod_type;
    if (ilog2_exact(N) < 6 || ilog2_exact(N) > 12)
        return fail(OFDM_ERR_UNSUPPORTED, "fft_size=%ld: the HIP FFT covers powers of two 64..4096", N);
    if (P < 1 || D < P || D % P)
        return fail(OFDM_ERR_UNSUPPORTED, "num_data_subc=%ld must be a positive multiple of num_pilot_subc=%ld", D,
                    P);
    if (P > 256) return fail(OFDM_ERR_UNSUPPORTED, "num_pilot_subc > 256");
    if (!(k == 1 || k == 2 || k == 4 || k == 6 || k == 8))
        return fail(OFDM_ERR_INVALID, "modType=%ld is not one of 1,2,4,6,8 (OFDM/modulation.hpp:11-17)", k);
    if (p->cp_size < 0 || p->cp_size > N) return fail(OFDM_ERR_INVALID, "cp_size out of range");
    if (p->num_symb < 1 || p->num_pr_symb < 1) return fail(OFDM_ERR_INVALID, "num_symb/num_pr_symb must be >= 1");
    if ((D * p->num_symb * k) % 8 || (D * k) % 8)
        return fail(OFDM_ERR_UNSUPPORTED, "num_data_subc*modType must be a multiple of 8 bits");
    if ((D * p->num_pr_symb) % 8) return fail(OFDM_ERR_UNSUPPORTED, "preamble bits must fill bytes");
    // the layout must stay inside [1, N) without collisions
    tables::Layout lay;
    if (const char* why = tables::carrier_layout(N, D, P, lay)) return fail(OFDM_ERR_INVALID, "%s", why);
    if (p->t2sin_size < 0 || (p->t2sin_size && (p->t2_sin_f1 < 0 || p->t2_sin_f1 >= p->t2sin_size ||
                                                p->t2_sin_f2 < 0 || p->t2_sin_f2 >= p->t2sin_size)))
        return fail(OFDM_ERR_INVALID, "T2 tones outside T2sin_size");
    if (p->pr_sin_len < 0 || p->pr_sin_len > (N + p->cp_size) * p->num_pr_symb)
        return fail(OFDM_ERR_INVALID, "pr_sin_len exceeds the preamble");
    return OFDM_OK;
}

// ---- the steps of ofdm_create, in the order of their device work ----

void set_geometry(ofdm_ctx* c, const ofdm_params& p)
{
    c->p = p;
    c->N = (int)p.fft_size;
    c->logn = ilog2_exact(c->N);
    c->D = (int)p.num_data_subc;
    c->P = (int)p.num_pilot_subc;
    c->cp = (int)p.cp_size;
    c->S = (int)p.num_symb;
    c->k = (int)p.mod_type;
    c->L = c->N + c->cp;
    c->seg = c->D / c->P;
    c->npr = (int)p.num_pr_symb;
    c->t2 = (int)p.t2sin_size;
    c->geo = tables::geometry(p);
    ofdm_walk_tuning_default(&c->walk);
    c->ring = std::max(0L, p.rx_buf_size) * c->geo.frame_len;  // rx.cpp:53 / sdr.hpp:141
}

// the carrier layout, the per-thread tables the kernels read it through, the
// twiddles and the constellations
int layout_tables(ofdm_ctx* c)
{
    tables::Layout lay;
    if (const char* why = tables::carrier_layout(c->N, c->D, c->P, lay)) return fail(OFDM_ERR_INVALID, "%s", why);
    for (int j = 0; j < c->P; ++j) {
        c->geo.pilot_bin[j] = lay.pilot[j];
        c->geo.segment_bin[j] = lay.segst[j];
    }
    c->tx_code = tables::tx_code(lay);
    c->tx_dead = ofdm::tx_dead_masks(c->tx_code);
    int rc;
    if (std::any_of(c->tx_dead.begin(), c->tx_dead.end(), [](unsigned m) { return m != 0; }) &&
        (rc = upload(c->d_tx_dead, c->tx_dead)))
        return rc;
    if ((rc = upload(c->d_rx_pack, tables::rx_pack(lay, c->N))) ||
        (rc = upload(c->d_pilot_swz, tables::pilot_swz(lay, c->N))) || (rc = upload(c->d_tx_code, c->tx_code)) ||
        (rc = upload(c->d_tw, twiddles(c->N))) || (rc = upload(c->d_data_bin, lay.data_bin)) ||
        (rc = upload(c->d_data_slot, lay.data_slot)) || (rc = upload(c->d_pilot_bin, lay.pilot)) ||
        (rc = upload(c->d_bin_map, lay.bin_map)) || (rc = upload(c->d_const, tables::constellation(c->k))) ||
        (rc = upload(c->d_const_bpsk, tables::constellation(1))))
        return rc;
    return OFDM_OK;
}

// decide_select's thresholds, found on the device
int decision_thresholds(ofdm_ctx* c)
{
    if (c->k != 2) return OFDM_OK;  // the rx emit's fast path takes QPSK only (16-QAM measured no gain)
    DevBuf<double> d_tau;
    double h_tau[4] = {};
    hipError_t e = hipMalloc((void**)d_tau.put(), sizeof(h_tau));
    if (e == hipSuccess) e = ofdm::launch_decide_tau_scan(c->k, d_tau, nullptr);
    if (e == hipSuccess) e = hipMemcpy(h_tau, d_tau, sizeof(h_tau), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "decision threshold scan");
    for (int j = 0; j < 3; ++j) c->dec_tau[j] = h_tau[j];
    c->dec_fast = h_tau[3] == 1.0;
    return OFDM_OK;
}

// PREAMBLE_FORM (Frame.cpp:259-294): the BPSK OFDM symbol(s) of the preamble
// bytes, made by the tx kernel itself
int synthesize_preamble(ofdm_ctx* c)
{
    const long nb = (long)c->D * c->npr / 8, plen = c->geo.preamble_len;
    c->preamble_bytes = tables::preamble_bytes(nb, c->p.pr_seed);
    DevBuf<uint8_t> d_b;
    DevBuf<double2> d_pre;
    HIP_TRY(hipMalloc((void**)d_b.put(), std::max<long>(1, nb)));
    HIP_TRY(hipMalloc((void**)d_pre.put(), plen * sizeof(double2)));
    HIP_TRY(hipMemcpy(d_b, c->preamble_bytes.data(), nb, hipMemcpyHostToDevice));
    ofdm::TxArgs a{};
    a.tab = c->tables(true);
    a.bytes = d_b;
    a.iq = d_pre;
    a.nframes = 1;
    a.frame_stride = plen;
    a.S = c->npr;
    a.D = c->D;
    a.P = c->P;
    a.cp = c->cp;
    a.k = 1;
    a.bytes_per_frame = nb;
    a.pilot_ampl = (double)c->p.pilot_ampl / 1000;
    a.inv_sqrt_n = 1.0 / std::sqrt((double)c->N);
    a.mult = (double)c->p.mult;
    hipError_t e = ofdm::launch_tx(c->logn, a, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<double2> pre(plen);
    if (e == hipSuccess) e = hipMemcpy(pre.data(), d_pre, plen * sizeof(double2), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "preamble synthesis");
    c->ofdm_preamble.resize(plen);
    for (long i = 0; i < plen; ++i) c->ofdm_preamble[i] = cd(pre[i].x, pre[i].y);
    return OFDM_OK;
}

// what the detectors and the channel estimate take from the preamble and the
// T2 symbol: the frame header, the BPSK points, the correlation template and
// (where the walker's FFT search covers its length) the template's spectrum
int preamble_tables(ofdm_ctx* c)
{
    const ofdm_params& p = c->p;
    c->t2_symbol = tables::t2_symbol(c->t2, p.t2_sin_f1, p.t2_sin_f2);
    c->t2_mask = tables::t2_mask(c->t2, (int)p.t2_sin_f1, (int)p.t2_sin_f2, (int)p.smooth);
    c->mod_preamble = tables::mod_preamble(c->preamble_bytes, (long)c->D * c->npr);
    c->templ = tables::preamble_template(c->ofdm_preamble, (int)p.pr_sin_len);
    std::vector<double2> hdr = as_double2(c->t2_symbol);
    const std::vector<double2> pre = as_double2(c->ofdm_preamble);
    hdr.insert(hdr.end(), pre.begin(), pre.end());
    std::vector<double2> tsp, twm;
    if (p.pr_sin_len <= ofdm::WALK_FFT_M - 63) {  // windows of >= 64 lags
        tsp = tables::template_spectrum(c->templ, ofdm::WALK_FFT_M, &c->tspec_max);
        twm = twiddles(ofdm::WALK_FFT_M);
    }
    std::vector<float2> tsp32(tsp.size());
    for (size_t k = 0; k < tsp.size(); ++k) tsp32[k] = make_float2((float)tsp[k].x, (float)tsp[k].y);
    int rc;
    if ((!tsp.empty() &&
         ((rc = upload(c->d_tspec, tsp)) || (rc = upload(c->d_tspec32, tsp32)) || (rc = upload(c->d_twm, twm)))) ||
        (rc = upload(c->d_header, hdr)) || (rc = upload(c->d_preamble, pre)) ||
        (rc = upload(c->d_templ, as_double2(c->templ))) || (rc = upload(c->d_modpre, as_double2(c->mod_preamble))) ||
        (rc = upload(c->d_t2mask, c->t2_mask)))
        return rc;
    return OFDM_OK;
}

int detector_scratch(ofdm_ctx* c)
{
    int rc;
    // T2 detector scratch {min block = INT_MAX, done count = 0} (left so by
    // every t2_scan launch), word 2: preamble_corr's start index
    if ((rc = upload(c->d_first, std::vector<int>{INT_MAX, 0, 0, 0}))) return rc;
    // find_preamble's split scratch for up to PRE_SCRATCH_STARTS start indices
    // (counters zero between launches); more starts per call take the
    // one-workgroup form, so the entry point never allocates
    const size_t cyc = 2 * (size_t)c->p.t2sin_size + (size_t)c->p.pr_sin_len;
    if ((rc = upload(c->d_pre_hv, std::vector<double>(ofdm_ctx::PRE_SCRATCH_STARTS * cyc, 0.0))) ||
        (rc = upload(c->d_pre_done, std::vector<unsigned>(ofdm_ctx::PRE_SCRATCH_STARTS, 0u))))
        return rc;
    if (c->t2 >= 64 && c->t2 <= 4096 && ilog2_exact(c->t2) > 0) {
        c->t2_logn = ilog2_exact(c->t2);
        if ((rc = upload(c->d_t2tw, twiddles(c->t2)))) return rc;
    }
    return OFDM_OK;
}

// rx dynamic-frame counters: zero now, and left zero by every rx launch
int rx_counters(ofdm_ctx* c)
{
    const size_t qbytes = ofdm_ctx::RX_QUEUE_SLOTS * 16 * sizeof(int);
    hipError_t qe = hipMalloc((void**)c->d_rxq.put(), qbytes);
    if (qe == hipSuccess) qe = hipMemset(c->d_rxq, 0, qbytes);
    if (qe == hipSuccess) qe = hipDeviceSynchronize();
    if (qe != hipSuccess) return hip_fail(qe, "rx frame counters");
    return OFDM_OK;
}

}  // namespace

// pilot_freq_sinh plan for a form of nsym symbols: S = (N+cp)*nsym = M or 5*M,
// M = 2^m. A new form length builds and uploads its tables (allocation, host
// copies): `st` is the stream the caller will launch on, refused while it is
// being captured.
int ofdm::cfo_plan(ofdm_ctx* c, int nsym, ofdm_ctx::CfoPlan** out, hipStream_t st)
{
    for (auto& pl : c->cfo_plans)
        if (pl.nsym == nsym) {
            *out = &pl;
            return OFDM_OK;
        }
    if (capturing(st)) return capture_refused("the tables of a new CFO form length");
    const long S = (long)c->L * nsym;
    ofdm_ctx::CfoPlan pl;
    pl.nsym = nsym;
    if (!tables::cfo_shape(S, &pl.g, &pl.logm))
        return fail(OFDM_ERR_UNSUPPORTED, "pilot_freq_sinh: form length %ld is not 2^a or 5*2^a (64 <= 2^a <= %d)", S,
                    4096);
    const std::vector<int> borders = tables::cfo_borders(c->N, c->D, c->P, S);
    for (int b : borders)
        if (b < 0 || b > S) return fail(OFDM_ERR_UNSUPPORTED, "pilot_freq_sinh windows leave the spectrum");
    int rc;
    if ((rc = upload(pl.tw_sub, twiddles(1 << pl.logm))) || (rc = upload(pl.borders, borders))) return rc;
    if (pl.g == 5 && (rc = upload(pl.tw_full, twiddles((int)S)))) return rc;
    c->cfo_plans.push_back(std::move(pl));
    *out = &c->cfo_plans.back();
    return OFDM_OK;
}

extern "C" {

int ofdm_params_default(ofdm_params* o)
{
    if (!o) return fail(OFDM_ERR_INVALID, "null params");
    *o = ofdm_params{};
    o->fft_size = 512;
    o->num_data_subc = 256;
    o->num_pilot_subc = 8;
    o->cp_size = 128;
    o->num_symb = 8;
    o->num_pr_symb = 1;
    o->pr_sin_len = 128;
    o->pr_seed = 42;
    o->pr_level = 500;
    o->t2sin_size = 256;
    o->t2_sin_f1 = 17;
    o->t2_sin_f2 = 51;
    o->t2_sin_level = 800;
    o->smooth = 5;
    o->mod_type = 4;
    o->pilot_ampl = 2500;
    o->mult = 200;
    o->rx_buf_size = 40;
    o->iterations = 10000;
    return OFDM_OK;
}

int ofdm_params_from_config(const char* path, ofdm_params* o)
{
    if (!o) return fail(OFDM_ERR_INVALID, "null params");
    std::unordered_map<std::string, long> c;
    int rc = parse_file(path, c);
    if (rc) return rc;
    // ConfigMap::operator[] semantics: missing keys read as 0
    o->fft_size = c["fft_size"];
    o->num_data_subc = c["num_data_subc"];
    o->num_pilot_subc = c["num_pilot_subc"];
    o->cp_size = c["cp_size"];
    o->num_symb = c["num_symb"];
    o->num_pr_symb = c["num_pr_symb"];
    o->pr_sin_len = c["pr_sin_len"];
    o->pr_seed = c["pr_seed"];
    o->pr_level = c["pr_level"];
    o->t2sin_size = c["T2sin_size"];
    o->t2_sin_f1 = c["T2_sin_f1"];
    o->t2_sin_f2 = c["T2_sin_f2"];
    o->t2_sin_level = c["T2_sin_level"];
    o->smooth = c["smooth"];
    o->mod_type = c["modType"];
    o->pilot_ampl = c["pilot_ampl"];
    o->mult = c["mult"];
    o->rx_buf_size = c["rx_buf_size"];
    o->iterations = c["iterations"];
    return OFDM_OK;
}

int ofdm_config_lookup(const char* path, const char* key, long* value)
{
    if (!key || !value) return fail(OFDM_ERR_INVALID, "null key/value");
    std::unordered_map<std::string, long> c;
    int rc = parse_file(path, c);
    if (rc) return rc;
    *value = c[key];
    return OFDM_OK;
}

int ofdm_create(const ofdm_params* params, int device, ofdm_ctx** out)
{
    if (!params || !out) return fail(OFDM_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc = validate(params);
    if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(OFDM_ERR_HIP, "no HIP device available (the modem core has no CPU path)");
    if (device < 0 || device >= ndev) return fail(OFDM_ERR_INVALID, "device %d out of range", device);
    HIP_TRY(hipSetDevice(device));

    std::unique_ptr<ofdm_ctx> c(new ofdm_ctx);  // a failed step deletes it, and with it what the steps before made
    c->device = device;
    set_geometry(c.get(), *params);
    if ((rc = layout_tables(c.get())) || (rc = decision_thresholds(c.get())) || (rc = synthesize_preamble(c.get())) ||
        (rc = preamble_tables(c.get())) || (rc = detector_scratch(c.get())) || (rc = rx_counters(c.get())))
        return rc;
    *out = c.release();
    return OFDM_OK;
}

int ofdm_destroy(ofdm_ctx* c)
{
    if (!c) return OFDM_OK;
    (void)hipSetDevice(c->device);
    delete c;
    return OFDM_OK;
}

}  // extern "C"
