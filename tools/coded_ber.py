#!/usr/bin/env python3
"""coded_ber.py — the coded link on the GPU (there is no CPU path: without a
device this fails). Config B (8192 frames, QPSK) and config C (4096 frames,
16-QAM), one rate-1/2, 2/3 or 3/4 codeword per frame (fec_max_info_bits of the
frame capacity), over a handful of noise levels:

  payload -> fec_encode -> tx with fused AWGN -> rx_soft (int8 and float32
  LLRs, bytes_out counted against the coded bytes: the uncoded BER) ->
  fec_decode (counted against the payload: the coded BER)

and the time per launch of the decoder (both predecessor-gather variants,
OFDM_FEC_GATHER unset / "lds"), the encoder and ofdm_rx_demod_soft on the
same frames: one process, after a warm-up, the legs alternating within each
repeat, one launch timed by HIP events at a time.

  python tools/coded_ber.py [--repeats 7] [--out profiles/coded_ber.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "c-ofdm_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import oracle as O  # noqa: E402  (config dicts only)

RATE_NAMES = {0: "1/2", 1: "2/3", 2: "3/4"}
# noise std relative to the rms of the noiseless tx samples, and the int8 LLR scale
SETUPS = {"B": (O.CONFIG_B, 8192, (0.4, 0.5, 0.6, 0.7, 0.8), 8.0),
          "C": (O.CONFIG_C, 4096, (0.14, 0.18, 0.22, 0.26, 0.30), 40.0)}


def summarise(ms):
    ms = [float(x) for x in ms]
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(float(np.median(ms)), 4),
            "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4)}


class Link:
    def __init__(self, name):
        import torch
        import ofdm_mi355x as M
        self.torch, self.M = torch, M
        self.name = name
        self.p, self.nf, self.noises, self.scale8 = SETUPS[name]
        self.m = M.Modem(self.p, 0)
        self.g = O.geometry(self.p)
        self.k = self.p["mod_type"]
        self.cap = self.g["bytes_per_frame"] * 8
        nf, g = self.nf, self.g
        self.iq = torch.empty((nf * g["message_len"],), dtype=torch.complex128, device="cuda")
        self.coded = torch.empty((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
        self.hard = torch.empty_like(self.coded)
        self.llr8 = torch.empty((nf * self.cap,), dtype=torch.int8, device="cuda")
        self.llr32 = torch.empty((nf * self.cap,), dtype=torch.float32, device="cuda")
        self.errs = torch.zeros((1,), dtype=torch.int64, device="cuda")
        self.info = {}
        for rate in RATE_NAMES:
            nb = M.fec_max_info_bits(self.cap, rate)
            nbytes = (nb + 7) // 8
            self.info[rate] = (nb, torch.randint(0, 256, (nf * nbytes,), dtype=torch.uint8, device="cuda"),
                               torch.empty((nf * nbytes,), dtype=torch.uint8, device="cuda"))
        wsz = max(M.fec_workspace_size(nf, nb) for nb, _, _ in self.info.values())
        self.ws = torch.empty((wsz,), dtype=torch.uint8, device="cuda") if wsz else None
        assert g["npts"] * self.k == self.cap
        # rms of the noiseless tx samples
        self.encode(0)
        self.m.tx(self.coded, nf, self.iq)
        self.rms = float(torch.sqrt(torch.mean(torch.abs(self.iq[:64 * g["message_len"]]) ** 2)).item())

    def encode(self, rate):
        nb, src, _ = self.info[rate]
        self.m.fec_encode(src, self.nf, nb, rate, self.coded, coded_stride=self.g["bytes_per_frame"])

    def count(self, fn):
        self.errs.zero_()
        fn(self.errs)
        self.torch.cuda.synchronize()
        return int(self.errs.item())

    def decode(self, rate, fmt, errs=None):
        nb, src, out = self.info[rate]
        llr = self.llr8 if fmt == self.M.LLR_I8 else self.llr32
        self.m.fec_decode(llr, self.nf, nb, rate, out, fmt=fmt, llr_stride=self.cap, workspace=self.ws,
                          ref=src if errs is not None else None, bit_errors=errs)

    def ber(self):
        M, rows = self.M, []
        for rel in self.noises:
            for rate in RATE_NAMES:
                nb = self.info[rate][0]
                self.encode(rate)
                self.m.tx(self.coded, self.nf, self.iq, noise_std=rel * self.rms, seed=17)
                unc = self.count(lambda e: self.m.rx_soft(self.iq, self.nf, self.llr8, self.scale8, M.LLR_I8,
                                                          bytes_out=self.hard, ref=self.coded, bit_errors=e))
                self.m.rx_soft(self.iq, self.nf, self.llr32, 1.0, M.LLR_F32)
                c8 = self.count(lambda e: self.decode(rate, M.LLR_I8, e))
                c32 = self.count(lambda e: self.decode(rate, M.LLR_F32, e))
                rows.append({"noise_rel": rel, "snr_db": round(-20 * math.log10(rel), 2), "rate": RATE_NAMES[rate],
                             "info_bits": nb, "coded_bits": M.fec_coded_bits(nb, rate),
                             "uncoded_bit_errors": unc, "uncoded_ber": unc / (self.nf * self.cap),
                             "coded_bit_errors_i8": c8, "coded_ber_i8": c8 / (self.nf * nb),
                             "coded_bit_errors_f32": c32, "coded_ber_f32": c32 / (self.nf * nb)})
                print(self.name, json.dumps(rows[-1]), flush=True)
        return rows

    def timing(self, repeats, warmup):
        torch, M = self.torch, self.M
        st = torch.cuda.current_stream()
        # LLRs of a working link (the second noise level), rate 1/2 coded bytes in the frames
        self.encode(0)
        self.m.tx(self.coded, self.nf, self.iq, noise_std=self.noises[1] * self.rms, seed=17)
        self.m.rx_soft(self.iq, self.nf, self.llr8, self.scale8, M.LLR_I8)
        self.m.rx_soft(self.iq, self.nf, self.llr32, 1.0, M.LLR_F32)

        def gather(variant, fn):
            def run():
                if variant:
                    os.environ["OFDM_FEC_GATHER"] = variant
                try:
                    fn()
                finally:
                    os.environ.pop("OFDM_FEC_GATHER", None)
            return run

        legs = {"rx_soft_i8": lambda: self.m.rx_soft(self.iq, self.nf, self.llr8, self.scale8, M.LLR_I8,
                                                     bytes_out=self.hard),
                "encode_r12": lambda: self.encode(0)}
        for rate, rn in RATE_NAMES.items():
            tag = "r" + rn.replace("/", "")
            legs[f"decode_i8_{tag}_bpermute"] = gather("", lambda rate=rate: self.decode(rate, M.LLR_I8))
            legs[f"decode_i8_{tag}_lds_pair"] = gather("lds", lambda rate=rate: self.decode(rate, M.LLR_I8))
        legs["decode_f32_r12_bpermute"] = gather("", lambda: self.decode(0, M.LLR_F32))
        legs["decode_f32_r12_lds_pair"] = gather("lds", lambda: self.decode(0, M.LLR_F32))
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
        res = {n: summarise(t) for n, t in times.items()}
        steps = self.nf * (self.info[0][0] + 6)
        d = res["decode_i8_r12_bpermute"]["median_ms"]
        res["summary"] = {
            "decode_i8_r12_over_rx_soft_i8": round(d / res["rx_soft_i8"]["median_ms"], 3),
            "decode_i8_r12_ns_per_trellis_step_per_codeword": round(d * 1e6 / (self.info[0][0] + 6), 3),
            "decode_i8_r12_trellis_steps_per_s": round(steps / d * 1e3, 0),
            "decode_i8_r12_info_bits_per_s": round(self.nf * self.info[0][0] / d * 1e3, 0),
            "lds_pair_over_bpermute_i8_r12": round(res["decode_i8_r12_lds_pair"]["median_ms"] / d, 3),
            "lds_pair_over_bpermute_f32_r12": round(res["decode_f32_r12_lds_pair"]["median_ms"]
                                                    / res["decode_f32_r12_bpermute"]["median_ms"], 3),
        }
        for n, r in res.items():
            print(self.name, n, json.dumps(r if n == "summary" else {k: r[k] for k in ("median_ms", "min_ms", "max_ms")}),
                  flush=True)
        return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7, help="timed repeats per leg (at least 5)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coded_ber.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("coded_ber.py needs a GPU (the modem core has no CPU path)")
    torch.manual_seed(1)  # the payloads
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "configs": []}
    soft = os.path.join(ROOT, "profiles", "soft_demap.json")
    if os.path.exists(soft):  # the committed soft-rx figure for the same frames, for the reader
        with open(soft) as f:
            legs = json.load(f)["configs"][0]["legs"]
        result["soft_demap_json_B_rx_soft_i8_median_ms"] = legs["b_rx_soft_i8_bytes"]["median_ms"]
    for name in SETUPS:
        link = Link(name)
        result["configs"].append({"config": name, "frames": link.nf, "k": link.k, "frame_capacity_bits": link.cap,
                                  "llr_scale_i8": link.scale8, "tx_rms": link.rms,
                                  "ber": link.ber(), "timing": link.timing(args.repeats, args.warmup)})
        link.m.close()
        del link
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
