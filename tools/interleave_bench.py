#!/usr/bin/env python3
"""interleave_bench.py — the interleaver and the scrambler on the GPU (there
is no CPU path: without a device this fails), on the frames of coded_ber.py:
config B (8192 frames, QPSK) and config C (4096 frames, 16-QAM), one codeword
per frame, the per-symbol block of ofdm_interleave_default.

Timing: every new kernel against ofdm_copy of the same byte count, and the
LLR deinterleave beside ofdm_fec_decode (int8, rate 1/2) on the same LLRs: one
process, after a warm-up, the legs alternating within each repeat, one launch
timed by HIP events at a time.

BER (config C, the noise levels of profiles/coded_ber.json, int8 LLRs): the
coded link with and without the interleaver, on the AWGN channel alone and
with a notch (1 % of the carriers, adjacent, their LLRs erased in every
symbol).

  python tools/interleave_bench.py [--repeats 7] [--out profiles/interleave.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "c-ofdm_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from coded_ber import RATE_NAMES, SETUPS, Link, summarise  # noqa: E402


class IlLink(Link):
    def __init__(self, name):
        super().__init__(name)
        torch, M = self.torch, self.M
        self.block = self.m.interleave_default()
        self.nsym = self.nf * self.p["num_symb"]
        assert self.block[0] * self.p["num_symb"] == self.cap
        self.sent = torch.empty_like(self.coded)
        self.llr8_d = torch.empty_like(self.llr8)
        self.llr32_d = torch.empty_like(self.llr32)
        self.scr = torch.empty_like(self.info[0][1])
        self.IL_F, self.IL_I = M.IL_FORWARD, M.IL_INVERSE

    # ---- BER
    def point(self, rel, rate, interleaved, notch):
        """Coded bit errors of one (noise, rate) point, int8 LLRs."""
        M, m = self.M, self.m
        nb, src, out = self.info[rate]
        self.encode(rate)
        tx_bytes = self.coded
        if interleaved:
            m.interleave_bits(self.coded, self.nsym, self.sent, self.IL_F)
            tx_bytes = self.sent
        m.tx(tx_bytes, self.nf, self.iq, noise_std=rel * self.rms, seed=17)
        m.rx_soft(self.iq, self.nf, self.llr8, self.scale8, M.LLR_I8)
        if notch:
            d = self.p["num_data_subc"]
            first = d // 3
            self.llr8.view(self.nsym, d, self.k)[:, first:first + notch, :] = 0
        llr = self.llr8
        if interleaved:
            m.interleave_llr(self.llr8, self.nsym, self.llr8_d, self.IL_I, fmt=M.LLR_I8)
            llr = self.llr8_d
        return self.count(lambda e: m.fec_decode(llr, self.nf, nb, rate, out, fmt=M.LLR_I8, llr_stride=self.cap,
                                                 workspace=self.ws, ref=src, bit_errors=e))

    def ber(self):
        rows = []
        notch = max(1, round(self.p["num_data_subc"] * 0.01))
        for rel in self.noises:
            for rate in RATE_NAMES:
                nb = self.info[rate][0]
                row = {"noise_rel": rel, "snr_db": round(-20 * math.log10(rel), 2), "rate": RATE_NAMES[rate],
                       "info_bits": nb, "notch_carriers": notch}
                for tag, width in (("awgn", 0), ("notch", notch)):
                    for il in (False, True):
                        e = self.point(rel, rate, il, width)
                        key = f"{tag}_{'interleaved' if il else 'plain'}"
                        row[key + "_bit_errors"] = e
                        row[key + "_ber"] = e / (self.nf * nb)
                rows.append(row)
                print(self.name, json.dumps(row), flush=True)
        return rows

    # ---- timing
    def timing(self, repeats, warmup):
        torch, M, m = self.torch, self.M, self.m
        st = torch.cuda.current_stream()
        self.encode(0)
        m.tx(self.coded, self.nf, self.iq, noise_std=self.noises[1] * self.rms, seed=17)
        m.rx_soft(self.iq, self.nf, self.llr8, self.scale8, M.LLR_I8)
        m.rx_soft(self.iq, self.nf, self.llr32, 1.0, M.LLR_F32)
        nb0, src0, _ = self.info[0]
        nbytes0 = (nb0 + 7) // 8
        sizes = {"bits": self.coded.numel(), "llr_i8": self.llr8.numel(), "llr_f32": self.llr32.numel() * 4,
                 "scramble": self.nf * nbytes0}
        legs = {
            "interleave_bits_fwd": lambda: m.interleave_bits(self.coded, self.nsym, self.sent, self.IL_F),
            "copy_bits": lambda: m.copy(self.sent, self.coded, sizes["bits"]),
            "deinterleave_llr_i8": lambda: m.interleave_llr(self.llr8, self.nsym, self.llr8_d, self.IL_I, fmt=M.LLR_I8),
            "interleave_llr_i8_fwd": lambda: m.interleave_llr(self.llr8, self.nsym, self.llr8_d, self.IL_F,
                                                              fmt=M.LLR_I8),
            "copy_llr_i8": lambda: m.copy(self.llr8_d, self.llr8, sizes["llr_i8"]),
            "deinterleave_llr_f32": lambda: m.interleave_llr(self.llr32, self.nsym, self.llr32_d, self.IL_I,
                                                             fmt=M.LLR_F32),
            "interleave_llr_f32_fwd": lambda: m.interleave_llr(self.llr32, self.nsym, self.llr32_d, self.IL_F,
                                                               fmt=M.LLR_F32),
            "copy_llr_f32": lambda: m.copy(self.llr32_d, self.llr32, sizes["llr_f32"]),
            "scramble": lambda: m.scramble(src0, self.nf, nb0, self.scr),
            "copy_scramble": lambda: m.copy(self.scr, src0, sizes["scramble"]),
            "decode_i8_r12": lambda: self.decode(0, M.LLR_I8),
        }
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
        med = {n: r["median_ms"] for n, r in res.items()}

        def gbs(nbytes, ms):  # read + write
            return round(2 * nbytes / ms / 1e6, 1)

        res["summary"] = {
            "bytes": sizes,
            "interleave_bits_fwd_over_copy": round(med["interleave_bits_fwd"] / med["copy_bits"], 3),
            "deinterleave_llr_i8_over_copy": round(med["deinterleave_llr_i8"] / med["copy_llr_i8"], 3),
            "interleave_llr_i8_fwd_over_copy": round(med["interleave_llr_i8_fwd"] / med["copy_llr_i8"], 3),
            "deinterleave_llr_f32_over_copy": round(med["deinterleave_llr_f32"] / med["copy_llr_f32"], 3),
            "interleave_llr_f32_fwd_over_copy": round(med["interleave_llr_f32_fwd"] / med["copy_llr_f32"], 3),
            "scramble_over_copy": round(med["scramble"] / med["copy_scramble"], 3),
            "deinterleave_llr_i8_GBps": gbs(sizes["llr_i8"], med["deinterleave_llr_i8"]),
            "copy_llr_i8_GBps": gbs(sizes["llr_i8"], med["copy_llr_i8"]),
            "deinterleave_llr_f32_GBps": gbs(sizes["llr_f32"], med["deinterleave_llr_f32"]),
            "copy_llr_f32_GBps": gbs(sizes["llr_f32"], med["copy_llr_f32"]),
            "deinterleave_llr_i8_over_decode_i8_r12": round(med["deinterleave_llr_i8"] / med["decode_i8_r12"], 4),
        }
        for n, r in res.items():
            print(self.name, n, json.dumps(r if n == "summary" else {k: r[k] for k in ("median_ms", "min_ms", "max_ms")}),
                  flush=True)
        return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7, help="timed repeats per leg (at least 5)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interleave.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("interleave_bench.py needs a GPU (the modem core has no CPU path)")
    torch.manual_seed(1)  # the payloads
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "configs": []}
    for name in SETUPS:
        link = IlLink(name)
        entry = {"config": name, "frames": link.nf, "k": link.k, "frame_capacity_bits": link.cap,
                 "block": list(link.block), "blocks": link.nsym, "timing": link.timing(args.repeats, args.warmup)}
        if name == "C":
            entry["llr_scale_i8"] = link.scale8
            entry["ber"] = link.ber()
        result["configs"].append(entry)
        link.m.close()
        del link
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
