#!/usr/bin/env python3
"""mac_bench.py — ofdm_mac_write / ofdm_mac_read on the GPU (there is no CPU
path: without a device this fails), 8192 frames per launch:

  B      config B's frame, frame_len = frame_stride = bytes_per_frame (1024)
  r12    the same frames as rate 1/2's info bytes: frame_len = 1023
         (floor(8186 / 8)), frame_stride = 1024
  packed frame_len = frame_stride = 1023: every second frame misaligned, the
         byte-per-lane path

Legs: mac_write and mac_read with both FCS kinds (read: payload, info and
frame_errors all asked for), beside ofdm_copy of the same bytes and
ofdm_scramble on the same buffers. One process, after a warm-up, the legs
alternating within each repeat, one launch timed by HIP events at a time.

--bench-headline also records bench.py's headline numbers (given on the
command line as measured: this tool does not run bench.py).

  python tools/mac_bench.py [--repeats 7] [--out profiles/mac.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "c-ofdm_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def summarise(ms):
    return {"ms": [round(t, 4) for t in ms], "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4)}


def run_case(torch, M, m, name, nf, frame_len, stride, repeats, warmup):
    u8 = torch.uint8
    st = torch.cuda.current_stream()
    caps = {fcs: M.mac_payload_len(frame_len, fcs) for fcs in (M.FCS_NONE, M.FCS_CRC32)}
    pstride = {fcs: (c + 3) // 4 * 4 if stride % 4 == 0 else c for fcs, c in caps.items()}
    payload = torch.randint(0, 256, (nf * (max(pstride.values())),), dtype=u8, device="cuda")
    frames = {fcs: torch.empty((nf * stride,), dtype=u8, device="cuda") for fcs in caps}
    back = torch.empty_like(payload)
    info = torch.empty((nf * 16,), dtype=u8, device="cuda")
    errs = torch.zeros((1,), dtype=torch.int64, device="cuda")
    other = torch.empty((nf * stride,), dtype=u8, device="cuda")
    nbits = frame_len * 8

    def write(fcs):
        m.mac_write(payload, caps[fcs], nf, frame_len, frames[fcs], fcs=fcs, tx_id=1, rx_id=2, seq0=0,
                    payload_stride=pstride[fcs], frame_stride=stride)

    def read(fcs):
        m.mac_read(frames[fcs], nf, frame_len, fcs=fcs, payload_out=back, info_out=info, frame_errors=errs,
                   expect_rx_id=2, frame_stride=stride, payload_stride=pstride[fcs])

    legs = {
        "mac_write_none": lambda: write(M.FCS_NONE),
        "mac_write_crc32": lambda: write(M.FCS_CRC32),
        "mac_read_none": lambda: read(M.FCS_NONE),
        "mac_read_crc32": lambda: read(M.FCS_CRC32),
        "copy": lambda: m.copy(other, frames[M.FCS_CRC32], nf * stride),
        "scramble": lambda: m.scramble(frames[M.FCS_CRC32], nf, nbits, other, in_stride=stride, out_stride=stride),
    }
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    assert int(errs.item()) == 0, "the frames just written must all pass"
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
    assert int(errs.item()) == 0
    res = {n: summarise(t) for n, t in times.items()}
    med = {n: r["median_ms"] for n, r in res.items()}
    nbytes = nf * stride
    res["summary"] = {"bytes": nbytes}
    for n in ("mac_write_none", "mac_write_crc32", "mac_read_none", "mac_read_crc32"):
        res["summary"][n + "_over_copy"] = round(med[n] / med["copy"], 3)
        res["summary"][n + "_over_scramble"] = round(med[n] / med["scramble"], 3)
        res["summary"][n + "_GBps"] = round(2 * nbytes / med[n] / 1e6, 1)  # read + write
    res["summary"]["copy_GBps"] = round(2 * nbytes / med["copy"] / 1e6, 1)
    for n, r in res.items():
        print(name, n, json.dumps(r if n == "summary" else {k: r[k] for k in ("median_ms", "min_ms", "max_ms")}),
              flush=True)
    return {"case": name, "frames": nf, "frame_len": frame_len, "frame_stride": stride, "timing": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7, help="timed repeats per leg (at least 5)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--bench-headline", default=None, help="JSON file with bench.py's parent / tree runs to record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mac.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("mac_bench.py needs a GPU (the modem core has no CPU path)")
    import ofdm_mi355x as M
    import oracle as O
    torch.manual_seed(1)
    m = M.Modem(dict(O.CONFIG_B), 0)
    bpf = O.geometry(dict(O.CONFIG_B))["bytes_per_frame"]
    nb = M.fec_max_info_bits(bpf * 8, M.FEC_R12)
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "cases": [
        run_case(torch, M, m, "B", args.frames, bpf, bpf, args.repeats, args.warmup),
        run_case(torch, M, m, "r12", args.frames, nb // 8, (nb + 7) // 8, args.repeats, args.warmup),
        run_case(torch, M, m, "packed", args.frames, nb // 8, nb // 8, args.repeats, args.warmup),
    ]}
    if args.bench_headline:
        with open(args.bench_headline) as f:
            result["bench_headline"] = json.load(f)
    m.close()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
