#!/usr/bin/env python3
"""Times x264gpu_picture_quality (the --psnr / --ssim pass, csrc/quality.hip) with device events: N pairs of WxH pictures, warm-up, then timed calls;
prints ms per call and TB/s of bytes read (both pictures of every pair) as one JSON line.  The measurement runs in a child process under its own
time limit; a child that fails or is cut off ends the tool with its status.
Usage: quality_time.py [--pairs 2048] [--size 1920x1080] [--calls 20] [--warmup 3] [--flags 3] [--limit 300]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from x264vfw_amd import lib
    w, h = (int(x) for x in a.size.split("x"))
    n, sz = a.pairs, w * h * 3 // 2
    torch.manual_seed(1)
    da = torch.randint(0, 256, (n * sz,), dtype=torch.uint8, device="cuda")
    db = da.clone()
    db[::5] ^= 6          # a fifth of the samples differ
    out = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call():
        lib.check(lib.x264gpu_picture_quality(da.data_ptr(), db.data_ptr(), n, w, h, a.flags, out.data_ptr(), st), "x264gpu_picture_quality")
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    first = out.cpu().numpy().copy()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.calls + 1)]
    ev[0].record()
    for i in range(a.calls):
        call()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(a.calls))
    assert (out.cpu().numpy() == first).all(), "the results changed between calls"
    med = ms[len(ms) // 2]
    print(json.dumps({"tool": "quality_time", "pairs": n, "size": a.size, "flags": a.flags, "calls": a.calls, "ms_per_call_median": round(med, 4), "ms_per_call_min": round(ms[0], 4),
                      "ms_per_call_max": round(ms[-1], 4), "bytes_read": 2 * n * sz, "tb_per_s": round(2 * n * sz / (med * 1e-3) / 1e12, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--flags", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds the measuring child may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    assert a.calls >= 1 and a.warmup >= 1
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
