"""Device time of x264gpu_gather_rows — N rows of a 1080p picture's quantiser offsets (32 640 bytes each) scattered over device memory into one [N][row] array —
next to the same rows as N x264gpu_memcpy_d2d calls: device events around each, the median of the repetitions after a warm-up, and the share of the 8 TB/s peak
(a copy reads and writes every byte: 2 x N x row bytes move).
usage: gather_time.py [--rows 2048 16] [--row-bytes 32640] [--reps 9]"""
import argparse, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import numpy as np, torch
from x264vfw_amd import lib

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="+", default=[2048, 16]); ap.add_argument("--row-bytes", type=int, default=32640); ap.add_argument("--reps", type=int, default=9)
a = ap.parse_args()
PEAK = 8e12
for n in a.rows:
    row = a.row_bytes
    slot = (row + 255) & ~255          # the members' arrays: slots of a ring, 256-byte aligned, one ring a member
    pool = torch.randint(0, 256, (n, 7 * slot), dtype=torch.uint8, device="cuda")
    ptrs = np.array([pool.data_ptr() + (s * 7 + (s * 3) % 7) * slot for s in range(n)], np.uint64)
    d_tab = torch.from_numpy(ptrs.view(np.int64)).cuda()
    d_dst = torch.zeros(n * row, dtype=torch.uint8, device="cuda")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3          # microseconds

    def gather():
        lib.check(lib.x264gpu_gather_rows(d_tab.data_ptr(), row, d_dst.data_ptr(), n, None), "gather")

    def copies():
        for s in range(n):
            lib.check(lib.x264gpu_memcpy_d2d(d_dst.data_ptr() + s * row, int(ptrs[s]), row, None), "d2d")
    out = {"rows": n, "row_bytes": row, "reps": a.reps}
    for name, fn in (("gather", gather), ("memcpy_d2d", copies)):
        timed(fn); timed(fn)
        us = sorted(timed(fn) for _ in range(a.reps))
        med = us[len(us) // 2]
        out[name] = {"us_median": round(med, 1), "us_min": round(us[0], 1), "us_max": round(us[-1], 1), "share_of_8TBps": round(2.0 * n * row / (med * 1e-6) / PEAK, 4)}
    want = torch.stack([pool.view(-1)[int(p) - pool.data_ptr():int(p) - pool.data_ptr() + row] for p in ptrs])
    gather(); torch.cuda.synchronize()
    out["equal"] = bool(torch.equal(d_dst.view(n, row), want))
    print(json.dumps(out))
