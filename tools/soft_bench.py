#!/usr/bin/env python3
"""soft_bench.py — what the soft-decision rx costs, measured on the GPU (there
is no CPU path: without a device this fails). Config B (8192 frames, QPSK) and
config C (4096 frames, 16-QAM), one process, after a warm-up, the legs
alternating within each repeat, one launch timed by HIP events at a time:

  a  ofdm_rx_demod with constell_out + bytes_out (the hard-decision rx)
  b  ofdm_rx_demod_soft, int8 LLRs + bytes_out, no constell_out
  c  as b with float32 LLRs
  d  the two-pass route: a, then ofdm_soft_demap (int8) on its constell_out
  e  ofdm_soft_demap alone (int8 and float32), beside a device-to-device copy
     that moves the same number of bytes

Per leg: every repeat's ms, median / min / max, the algorithmic bytes from the
shapes (rx input 16 B per sample of the N-sample bodies, 16 B per point of
constellation, k/8 B per point of bytes, k or 4k B per point of LLRs; leg d
also reads the constellation back), bytes/s and its share of the 8 TB/s peak.

  python tools/soft_bench.py [--repeats 7] [--out profiles/soft_demap.json]
                             [--headline FILE]   # bench.py A/B runs to embed
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "c-ofdm_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import oracle as O  # noqa: E402  (config dicts only)

PEAK = 8.0e12  # MI355X HBM3E bytes/s


def summarise(ms, nbytes):
    ms = [float(x) for x in ms]
    med = float(np.median(ms))
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4), "bytes": int(nbytes),
            "bytes_per_s": round(nbytes / med * 1e3, 0), "share_of_peak": round(nbytes / med * 1e3 / PEAK, 4)}


def run_config(name, p, nf, repeats, warmup):
    import torch
    import ofdm_mi355x as M

    m = M.Modem(p, 0)
    g = O.geometry(p)
    st = torch.cuda.current_stream()
    S, N, D, k = p["num_symb"], p["fft_size"], p["num_data_subc"], p["mod_type"]
    npts = nf * g["npts"]
    data = torch.randint(0, 256, (nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
    iq = torch.empty((nf * g["message_len"],), dtype=torch.complex128, device="cuda")
    m.tx(data, nf, iq, noise_std=0.2, seed=1)
    cons = torch.empty((npts,), dtype=torch.complex128, device="cuda")
    out = torch.empty_like(data)
    llr8 = torch.empty((npts * k,), dtype=torch.int8, device="cuda")
    llr32 = torch.empty((npts * k,), dtype=torch.float32, device="cuda")
    in_b = nf * S * 16 * N
    by_b = npts * k // 8
    flat8_b, flat32_b = npts * (16 + k), npts * (16 + 4 * k)
    c8a = torch.empty((flat8_b // 2,), dtype=torch.uint8, device="cuda")
    c8b = torch.empty_like(c8a)
    c32a = torch.empty((flat32_b // 2,), dtype=torch.uint8, device="cuda")
    c32b = torch.empty_like(c32a)

    def leg_d():
        m.rx(iq, nf, constell_out=cons, bytes_out=out)
        m.soft_demap(cons, npts, llr8, 4.0, M.LLR_I8)

    legs = {
        "a_rx_hard_constell_bytes": (lambda: m.rx(iq, nf, constell_out=cons, bytes_out=out), in_b + 16 * npts + by_b),
        "b_rx_soft_i8_bytes": (lambda: m.rx_soft(iq, nf, llr8, 4.0, M.LLR_I8, bytes_out=out), in_b + k * npts + by_b),
        "c_rx_soft_f32_bytes": (lambda: m.rx_soft(iq, nf, llr32, 4.0, M.LLR_F32, bytes_out=out),
                                in_b + 4 * k * npts + by_b),
        "d_two_pass_i8": (leg_d, in_b + 16 * npts + by_b + flat8_b),
        "e_soft_demap_i8": (lambda: m.soft_demap(cons, npts, llr8, 4.0, M.LLR_I8), flat8_b),
        "e_copy_same_bytes_as_i8": (lambda: c8b.copy_(c8a), 2 * c8a.numel()),
        "e_soft_demap_f32": (lambda: m.soft_demap(cons, npts, llr32, 4.0, M.LLR_F32), flat32_b),
        "e_copy_same_bytes_as_f32": (lambda: c32b.copy_(c32a), 2 * c32a.numel()),
    }
    m.rx(iq, nf, constell_out=cons, bytes_out=out)  # leg e's points
    for _ in range(warmup):
        for fn, _b in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in legs}
    for _ in range(repeats):
        evs = {}
        for n, (fn, _b) in legs.items():  # alternating: every leg once per repeat
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            evs[n] = (e0, e1)
        torch.cuda.synchronize()
        for n, (e0, e1) in evs.items():
            times[n].append(e0.elapsed_time(e1))
    res = {"config": name, "frames": nf, "k": k, "points": npts,
           "legs": {n: summarise(times[n], legs[n][1]) for n in legs}}
    L = res["legs"]
    a, b, d = L["a_rx_hard_constell_bytes"], L["b_rx_soft_i8_bytes"], L["d_two_pass_i8"]
    spread = max(a["spread_ms"], b["spread_ms"], d["spread_ms"])
    res["verdict"] = {
        "spread_ms": spread,
        "b_faster_than_d_beyond_spread": bool(d["median_ms"] - b["median_ms"] > spread),
        "b_no_slower_than_a_beyond_spread": bool(b["median_ms"] - a["median_ms"] <= spread),
        "flat_i8_vs_copy": round(L["e_soft_demap_i8"]["bytes_per_s"] / L["e_copy_same_bytes_as_i8"]["bytes_per_s"], 3),
        "flat_f32_vs_copy": round(L["e_soft_demap_f32"]["bytes_per_s"] / L["e_copy_same_bytes_as_f32"]["bytes_per_s"],
                                  3),
    }
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7, help="timed repeats per leg (at least 5)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_demap.json"))
    ap.add_argument("--headline", default="", help="JSON file with bench.py A/B runs, embedded as 'headline'")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("soft_bench.py needs a GPU (the modem core has no CPU path)")
    result = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK, "repeats": args.repeats,
              "configs": [run_config("B", O.CONFIG_B, 8192, args.repeats, args.warmup),
                          run_config("C", O.CONFIG_C, 4096, args.repeats, args.warmup)]}
    if args.headline:
        with open(args.headline) as f:
            result["headline"] = json.load(f)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    for c in result["configs"]:
        for n, leg in c["legs"].items():
            print(f"{c['config']} {n:28s} {leg['median_ms']:8.4f} ms  [{leg['min_ms']:.4f}, {leg['max_ms']:.4f}]  "
                  f"{leg['bytes_per_s'] / 1e12:6.3f} TB/s  {100 * leg['share_of_peak']:5.1f}% of peak")
        print(c["config"], json.dumps(c["verdict"]))


if __name__ == "__main__":
    main()
