// ofdm_csi.hpp — argument blocks and launchers of the frequency-selective
// channel path (ofdm_csi.hip), called from ofdm_capi.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include "ofdm_internal.hpp"

namespace ofdm {

constexpr int CSI_SMOOTH_MAX = 64;      // largest smoothing half-width
constexpr size_t CSI_LDS_MAX = 160 * 1024;

struct ChanLsArgs {
    DevTables tab;              // BPSK tables (the preamble is a BPSK symbol)
    const double2* x;           // preamble form
    long nframes, frame_stride;
    const double2* mod_pre;     // D*npr BPSK points
    double2* chan_out;          // nullable: H, D per frame
    double* csi_out;            // nullable: |H|^2, D per frame
    long chan_stride, csi_stride;
    int npr, D, P, cp, smooth;
    double pilot_ampl;
};

struct SoftCsiArgs {
    const double2* pts;         // nframes * npts equalised points
    const double* csi;          // D weights per frame
    const double* frame_scale;  // nullable, device: frame f uses scale * frame_scale[f]
    void* out;                  // nframes*npts*k LLRs
    long nframes, csi_stride;   // csi_stride 0: one shared vector
    int npts, D, k, fmt;        // npts = D * num_symb points per frame
    double scale;
};

// dynamic LDS of chan_ls_kernel for this geometry (bytes)
size_t chan_ls_lds_bytes(int logn, int npr, int D, int P);
hipError_t launch_chan_ls(int logn, const ChanLsArgs& a, hipStream_t st);
hipError_t launch_soft_demap_csi(const SoftCsiArgs& a, hipStream_t st);

}  // namespace ofdm
