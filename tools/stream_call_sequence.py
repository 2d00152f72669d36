#!/usr/bin/env python3
"""stream_call_sequence.py — the HIP calls a stream-receiver call makes, as an
ordered list, to compare two builds of the library (OFDM_MI355X_LIB) after a
change to the host orchestration that must not move a kernel, copy, memset,
event or wait.

  rocprofv3 --kernel-trace --hip-trace --memory-copy-trace --output-format csv -d DIR -o run -- \\
      python tools/stream_call_sequence.py run
  python tools/stream_call_sequence.py reduce DIR > sequence.txt
  python tools/stream_call_sequence.py compare a.txt b.txt

`run` makes three calls on config D, 40 frames (each once untimed first, so
that no scratch grows in the traced call), each between two pairs of device
synchronisations: a look-back call; a lookback = 0 call with halo_milli = 0
(the host stitch with re-walks); a look-back call with max_rec_cap = 1 (record
overflow, then the halo walk). `reduce` cuts the trace at those pairs and
prints, per call: the host's calls in issue order (launches, copies, memsets,
event records, waits, synchronisations), the kernels in start order with grid
and block, and the copies in start order (with their size where the trace
has one)."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = [("lookback", {}), ("host_stitch_rewalks", dict(lookback=0, halo_milli=0)),
         ("lookback_overflow", dict(max_rec_cap=1))]
API = ("hipLaunchKernel", "hipExtLaunchKernel", "hipModuleLaunchKernel", "hipExtModuleLaunchKernel",
       "hipMemsetAsync", "hipMemcpyAsync", "hipMemcpy", "hipEventRecord", "hipStreamWaitEvent",
       "hipEventSynchronize", "hipStreamSynchronize")
MARK = "hipDeviceSynchronize"


def run():
    sys.path.insert(0, os.path.join(ROOT, "c-ofdm_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import ofdm_mi355x as M
    import oracle as O
    from common import D, impaired_stream

    x, _ = impaired_stream(D, 40, seed=5, gap_max=6000)
    g, nf = O.geometry(D), 256
    m = M.Modem(D, 0)
    dx = torch.from_numpy(x).cuda()
    pbs = torch.zeros((nf,), dtype=torch.int64, device="cuda")
    out = torch.zeros((nf * g["bytes_per_frame"],), dtype=torch.uint8, device="cuda")
    cons = torch.zeros((nf * g["npts"],), dtype=torch.complex128, device="cuda")

    def call(tuning):
        m.walk_tuning(**tuning)
        return m.rx_stream(dx, len(x), nf, pb_out=pbs, bytes_out=out, constell_out=cons, chunk=9000)

    for _, tuning in CALLS:
        call(tuning)
    for name, tuning in CALLS:
        torch.cuda.synchronize()
        torch.cuda.synchronize()
        found = call(tuning)
        torch.cuda.synchronize()
        torch.cuda.synchronize()
        print(name, found, "frames", flush=True)
    m.close()


def rows(d, kind):
    paths = glob.glob(os.path.join(d, "**", "*_%s.csv" % kind), recursive=True)
    return [r for p in sorted(paths) for r in csv.DictReader(open(p))]


def reduce(d):
    api = sorted((r for r in rows(d, "hip_api_trace") if r["Function"] in API + (MARK,)),
                 key=lambda r: int(r["Start_Timestamp"]))
    # a call lies between two pairs of back-to-back device synchronisations
    spans, i = [], 0
    pairs = [k for k in range(len(api) - 1) if api[k]["Function"] == MARK and api[k + 1]["Function"] == MARK]
    for a, b in zip(pairs, pairs[1:]):
        seg = api[a + 2:b]
        if seg and all(r["Function"] != MARK for r in seg):
            spans.append((int(api[a + 1]["End_Timestamp"]), int(api[b]["Start_Timestamp"]), seg))
    spans = spans[-len(CALLS):]
    kernels = sorted(rows(d, "kernel_trace"), key=lambda r: int(r["Start_Timestamp"]))
    copies = sorted(rows(d, "memory_copy_trace"), key=lambda r: int(r["Start_Timestamp"]))
    for (name, _), (t0, t1, seg) in zip(CALLS, spans):
        print("== call: %s" % name)
        print("-- host calls in issue order")
        for r in seg:
            print(r["Function"])
        print("-- kernels in start order (name, grid, block)")
        for r in kernels:
            if t0 <= int(r["Start_Timestamp"]) <= t1:
                print("%s grid=(%s,%s,%s) block=(%s,%s,%s)" % (
                    r["Kernel_Name"].split("(")[0], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"],
                    r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"]))
        print("-- copies in start order (direction, bytes)")
        for r in copies:
            if t0 <= int(r["Start_Timestamp"]) <= t1:
                size = next((r[k] for k in ("Bytes", "Size", "bytes", "size") if k in r), "n/a")
                print("%s %s" % (r["Direction"], size))
    return 0 if len(spans) == len(CALLS) else 1


def compare(a, b):
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    print("%s: %d lines; %s: %d lines" % (a, len(la), b, len(lb)))
    diff = [(i + 1, x, y) for i, (x, y) in enumerate(zip(la, lb)) if x != y]
    for i, x, y in diff[:20]:
        print("line %d: %r != %r" % (i, x, y))
    same = not diff and len(la) == len(lb) and len(la) > 3 * len(CALLS)
    print("EQUAL" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    sys.exit(run() if cmd == "run" else reduce(sys.argv[2]) if cmd == "reduce" else compare(*sys.argv[2:4]))
