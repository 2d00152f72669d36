#!/usr/bin/env python3
"""selective_link.py — the frequency-selective channel path on the GPU (there
is no CPU path: without a device this fails).

Timing (config B, 8192 frames; one process, after a warm-up, the legs
alternating within each repeat, one launch timed by HIP events at a time):
ofdm_chan_estimate_ls against ofdm_chan_estimate on the same preamble forms,
and ofdm_soft_demap_csi against ofdm_soft_demap on the same points, both
formats.

Loss table (config D, 16-QAM, one codeword per frame, the frames of
tests/csi_model.py link_case: echo at 12 dB and notch at 18 dB, rates 1/2 and
2/3, int8 LLRs at scale 8, default interleaver) over three legs: the
unit-phasor estimate of ofdm_chan_estimate, the LS estimate with unweighted
LLRs, the LS estimate with ofdm_soft_demap_csi.

  python tools/selective_link.py [--repeats 7] [--frames 64] [--out profiles/selective_link.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (("c-ofdm_amd", "python"), ("oracle",), ("tools",), ("tests",)):
    sys.path.insert(0, os.path.join(ROOT, *d))

import csi_model as CM  # noqa: E402
import fec_model as F  # noqa: E402
import oracle as O  # noqa: E402
from coded_ber import RATE_NAMES, summarise  # noqa: E402
from common import TAPS_ECHO, TAPS_NOTCH  # noqa: E402

TIMING_FRAMES = 8192
TABLE = (("echo", TAPS_ECHO, 12.0), ("notch", TAPS_NOTCH, 18.0))


def alternate(torch, legs, repeats, warmup):
    st = torch.cuda.current_stream()
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in legs}
    for _ in range(repeats):
        evs = {}
        for n, fn in legs.items():  # alternating: every leg once per repeat
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            evs[n] = (e0, e1)
        torch.cuda.synchronize()
        for n, (e0, e1) in evs.items():
            times[n].append(e0.elapsed_time(e1))
    return {n: summarise(t) for n, t in times.items()}


def timing(torch, M, repeats, warmup):
    p = dict(O.CONFIG_B)
    m = M.Modem(p, 0)
    g = O.geometry(p)
    nf, Dn, k = TIMING_FRAMES, p["num_data_subc"], p["mod_type"]
    npre, npts = g["preamble_len"], g["npts"]
    # eight distinct noisy notch preambles, repeated over the batch
    case = CM.link_case(p, TAPS_NOTCH, F.R12, 8, 18.0)
    pre = torch.from_numpy(np.array(case["regions"][:, :npre], copy=True)).cuda()
    x = pre.repeat(nf // 8, 1).reshape(-1).contiguous()
    chan = torch.empty((nf * Dn,), dtype=torch.complex128, device="cuda")
    csi = torch.empty((nf * Dn,), dtype=torch.float64, device="cuda")
    pts = torch.view_as_complex(torch.rand((nf * npts, 2), dtype=torch.float64, device="cuda") * 3.0 - 1.5)
    llr32 = torch.empty((nf * npts * k,), dtype=torch.float32, device="cuda")
    llr8 = torch.empty((nf * npts * k,), dtype=torch.int8, device="cuda")
    m.chan_estimate_ls(x, nf, npre, chan, csi)
    legs = {
        "chan_estimate": lambda: m.chan_estimate(x, nf, npre, chan),
        "chan_estimate_ls": lambda: m.chan_estimate_ls(x, nf, npre, chan, csi),
        "chan_estimate_ls_chan_only": lambda: m.chan_estimate_ls(x, nf, npre, chan, None),
        "chan_estimate_ls_smooth3": lambda: m.chan_estimate_ls(x, nf, npre, chan, csi, smooth=3),
        "soft_demap_f32": lambda: m.soft_demap(pts, nf * npts, llr32, 8.0, M.LLR_F32),
        "soft_demap_csi_f32": lambda: m.soft_demap_csi(pts, nf, csi, llr32, 8.0, M.LLR_F32),
        "soft_demap_csi_f32_shared": lambda: m.soft_demap_csi(pts, nf, csi, llr32, 8.0, M.LLR_F32, csi_stride=0),
        "soft_demap_i8": lambda: m.soft_demap(pts, nf * npts, llr8, 8.0, M.LLR_I8),
        "soft_demap_csi_i8": lambda: m.soft_demap_csi(pts, nf, csi, llr8, 8.0, M.LLR_I8),
        "soft_demap_csi_i8_shared": lambda: m.soft_demap_csi(pts, nf, csi, llr8, 8.0, M.LLR_I8, csi_stride=0),
    }
    res = alternate(torch, legs, repeats, warmup)
    med = {n: r["median_ms"] for n, r in res.items()}
    res["summary"] = {
        "frames": nf, "preamble_bytes": nf * npre * 16, "points": nf * npts,
        "chan_estimate_ls_over_chan_estimate": round(med["chan_estimate_ls"] / med["chan_estimate"], 3),
        "chan_estimate_ls_preamble_GBps": round(nf * npre * 16 / med["chan_estimate_ls"] / 1e6, 1),
        "chan_estimate_preamble_GBps": round(nf * npre * 16 / med["chan_estimate"] / 1e6, 1),
        "soft_demap_csi_over_soft_demap_f32": round(med["soft_demap_csi_f32"] / med["soft_demap_f32"], 3),
        "soft_demap_csi_over_soft_demap_i8": round(med["soft_demap_csi_i8"] / med["soft_demap_i8"], 3),
        "soft_demap_f32_GBps": round(nf * npts * (16 + 4 * k) / med["soft_demap_f32"] / 1e6, 1),
        "soft_demap_csi_f32_GBps": round(nf * npts * (16 + 4 * k) / med["soft_demap_csi_f32"] / 1e6, 1),
        "soft_demap_i8_GBps": round(nf * npts * (16 + k) / med["soft_demap_i8"] / 1e6, 1),
        "soft_demap_csi_i8_GBps": round(nf * npts * (16 + k) / med["soft_demap_csi_i8"] / 1e6, 1),
    }
    for n, r in res.items():
        print("B", n, json.dumps(r if n == "summary" else {q: r[q] for q in ("median_ms", "min_ms", "max_ms")}),
              flush=True)
    m.close()
    return res


def loss_table(torch, M, nf):
    p = dict(O.DEFAULT)
    m = M.Modem(p, 0)
    g = O.geometry(p)
    Dn, S, k = p["num_data_subc"], p["num_symb"], p["mod_type"]
    npre, n, npts = g["preamble_len"], g["preamble_len"] + g["message_len"], g["npts"]
    cap = g["bytes_per_frame"] * 8
    c128, u8 = torch.complex128, torch.uint8
    chan = torch.empty((nf * Dn,), dtype=c128, device="cuda")
    csi = torch.empty((nf * Dn,), dtype=torch.float64, device="cuda")
    cons = torch.empty((nf * npts,), dtype=c128, device="cuda")
    llr = torch.empty((nf * cap,), dtype=torch.int8, device="cuda")
    dellr = torch.empty_like(llr)
    rows = []
    for tag, taps, snr in TABLE:
        for rate in (F.R12, F.R23):
            case = CM.link_case(p, taps, rate, nf, snr)
            nb = case["info_bits"]
            nbytes = (nb + 7) // 8
            x = torch.from_numpy(np.array(case["regions"], copy=True).reshape(-1)).cuda()
            ref = torch.from_numpy(F.pack(case["info"]).reshape(-1)).cuda()
            dec = torch.empty((nf * nbytes,), dtype=u8, device="cuda")
            wsz = M.fec_workspace_size(nf, nb)
            ws = torch.empty((wsz,), dtype=u8, device="cuda") if wsz else None
            row = {"channel": tag, "snr_db": snr, "rate": RATE_NAMES[rate], "frames": nf, "info_bits": nb}
            for leg in ("unit_phasor", "ls_unweighted", "ls_csi"):
                if leg == "unit_phasor":
                    m.chan_estimate(x, nf, n, chan)
                else:
                    m.chan_estimate_ls(x, nf, n, chan, csi)
                m.rx(x[npre:], nf, frame_stride=n, chan=chan, chan_stride=Dn, constell_out=cons)
                if leg == "ls_csi":
                    m.soft_demap_csi(cons, nf, csi, llr, 8.0, M.LLR_I8)
                else:
                    m.soft_demap(cons, nf * npts, llr, 8.0, M.LLR_I8)
                m.interleave_llr(llr, nf * S, dellr, M.IL_INVERSE, fmt=M.LLR_I8)
                e = torch.zeros((1,), dtype=torch.int64, device="cuda")
                m.fec_decode(dellr, nf, nb, rate, dec, fmt=M.LLR_I8, llr_stride=cap, workspace=ws, ref=ref,
                             bit_errors=e)
                torch.cuda.synchronize()
                got = dec.cpu().numpy().reshape(nf, nbytes)
                lost = int(np.any(got != F.pack(case["info"]), axis=1).sum())
                row[leg + "_codewords_lost"] = lost
                row[leg + "_ber"] = int(e.item()) / (nf * nb)
            rows.append(row)
            print("D", json.dumps(row), flush=True)
    m.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7, help="timed repeats per leg (at least 5)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64, help="frames of each row of the loss table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selective_link.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("selective_link.py needs a GPU (the modem core has no CPU path)")
    import ofdm_mi355x as M
    torch.manual_seed(1)  # the timing legs' points
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "timing": {"config": "B", "legs": timing(torch, M, args.repeats, args.warmup)},
              "loss_table": {"config": "D", "llr": "int8, scale 8", "rows": loss_table(torch, M, args.frames)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
